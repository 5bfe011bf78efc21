// Host constants of the single-device entries that the test build can replace, the door in front of every checked HIP call (pmx_ctx.hpp: hip_inject), and the test build's
// door to the strided hash kernel and its view of the pass-scratch pool (include/poseidon_mi355x_testing.h).  Compiled twice
// (Makefile): build/pmx_hooks.o for libposeidon_mi355x.so - the constants and nothing else, no hook symbol, no state - and
// build/pmx_hooks_test.o (-DPMX_TEST_HOOKS) for libposeidon_mi355x_test.so.  (The hooks of the device-group code live in pmx_mgpu.cpp.)
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <mutex>

#include "../../include/poseidon_mi355x.h"
#include "pmx_ctx.hpp"
#include "pmx_launch.hpp"

namespace pmx {
// Candidates per launch of pmx_sponge_grind (pmx_sponge.cpp), chosen from the sweep of profiles/grind/README.md.
static constexpr uint64_t kGrindChunk = (uint64_t)1 << 21;
// Leaves per piece of pmx_merkle_frontier_append / pmx_merkle_fixed (pmx_merkle.cpp); how it was chosen: profiles/merkle_fixed/README.md.
static constexpr uint64_t kMerkleFixedPiece = (uint64_t)1 << 22;
}  // namespace pmx

#ifdef PMX_TEST_HOOKS
static std::atomic<uint64_t> g_grind_chunk{0};   // 0: the product's
extern "C" int pmx_test_grind_chunk(uint64_t candidates) {
    g_grind_chunk.store(candidates);
    return PMX_OK;
}
uint64_t pmx::grind_chunk() {
    const uint64_t set = g_grind_chunk.load();
    return set ? set : kGrindChunk;
}
static std::atomic<uint64_t> g_matrix_slab_rows{0};   // 0: the product's (PMX_MATRIX_SLAB_BYTES)
extern "C" int pmx_test_matrix_slab_rows(uint64_t rows) {
    g_matrix_slab_rows.store(rows);
    return PMX_OK;
}
uint64_t pmx::matrix_slab_rows_hook() { return g_matrix_slab_rows.load(); }
static std::atomic<uint64_t> g_merkle_fixed_piece{0};   // 0: the product's
extern "C" int pmx_test_merkle_fixed_piece(uint64_t leaves) {
    g_merkle_fixed_piece.store(leaves);
    return PMX_OK;
}
uint64_t pmx::merkle_fixed_piece() {
    const uint64_t set = g_merkle_fixed_piece.load();
    return set ? set : kMerkleFixedPiece;
}
// The calling thread's checked HIP calls, counted from the last arm; the armed one is answered with hipErrorOutOfMemory, once, and not made.
// `note` is what hip_fail words the failure with, asked once: the checked calls of the unwinding (the event of a leased pool block) do
// not take it away, and a site that absorbs its failure (a registration, the record of a pool block's event) asks too, so that nothing
// is left behind for a later, real failure.
namespace {
struct HipInjector {
    int64_t armed = 0, calls = 0;
    bool pending = false;
    char note[256] = "";
};
thread_local HipInjector t_inject;
}  // namespace
hipError_t pmx::hip_inject(const char *what) {
    HipInjector &j = t_inject;
    if (++j.calls != j.armed) return hipSuccess;
    j.armed = 0;
    snprintf(j.note, sizeof j.note, "injected in place of %s", what);
    j.pending = true;
    return hipErrorOutOfMemory;
}
const char *pmx::hip_injected() {
    HipInjector &j = t_inject;
    if (!j.pending) return nullptr;
    j.pending = false;
    return j.note;
}
extern "C" int pmx_test_fail_hip(int64_t nth) {
    if (nth < 0) return pmx::set_error(PMX_ERR_ARG, "pmx_test_fail_hip: a negative count");
    HipInjector &j = t_inject;
    j.armed = nth;
    j.calls = 0;
    j.pending = false;
    j.note[0] = 0;
    return PMX_OK;
}
extern "C" int64_t pmx_test_hip_calls(void) { return t_inject.calls; }
extern "C" const char *pmx_test_hip_fired(void) { return t_inject.note; }
extern "C" int pmx_test_pass_pool(pmx_ctx *ctx, size_t *blocks, size_t *held, size_t *poisoned) {
    if (!ctx || !blocks || !held || !poisoned) return pmx::set_error(PMX_ERR_ARG, "pmx_test_pass_pool: null pointer");
    PMX_ABI_BEGIN("pmx_test_pass_pool")
    std::lock_guard<std::mutex> lock(ctx->pass_lock);
    *blocks = ctx->pass_pool.size();
    *held = *poisoned = 0;
    for (const pmx_ctx::PassBlock &b : ctx->pass_pool) {
        *held += !b.recorded;
        *poisoned += b.poisoned;
    }
    return PMX_OK;
    PMX_ABI_END
}
// the strided hash kernel of the matrix entries on the caller's own device buffers and stream, out_len = 1: enqueue only
extern "C" int pmx_test_matrix_leaves_dev(pmx_ctx *ctx, const uint64_t *d_matrix, size_t n_rows, size_t row_len, size_t row_stride, size_t elem_stride,
                                          uint64_t *d_leaves, void *stream) {
    if (!ctx || !d_matrix || !d_leaves) return pmx::set_error(PMX_ERR_ARG, "pmx_test_matrix_leaves_dev: null pointer");
    if (n_rows == 0 || row_len == 0 || n_rows > pmx::kMaxLaunchUnits) return pmx::set_error(PMX_ERR_ARG, "pmx_test_matrix_leaves_dev: bad shape");
    if (!pmx::aligned16(d_matrix) || !pmx::aligned16(d_leaves)) return pmx::set_error(PMX_ERR_ARG, "device pointers must be 16-byte aligned");
    PMX_BIND(ctx);
    PMX_HIP(pmx::launch_hash_strided(ctx->dev, ctx->t, d_matrix, row_len, row_stride, elem_stride, d_leaves, 1, n_rows, (hipStream_t)stream));
    return PMX_OK;
}
#else
hipError_t pmx::hip_inject(const char *) { return hipSuccess; }
const char *pmx::hip_injected() { return nullptr; }
uint64_t pmx::grind_chunk() { return kGrindChunk; }
uint64_t pmx::matrix_slab_rows_hook() { return 0; }
uint64_t pmx::merkle_fixed_piece() { return kMerkleFixedPiece; }
#endif
