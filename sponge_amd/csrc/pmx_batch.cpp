// C ABI of libposeidon_mi355x.so: the batch permutation and the batch hash, on device memory and - through the pinned pipeline - on host buffers.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/poseidon_mi355x.h"
#include "pmx_ctx.hpp"
#include "pmx_internal.hpp"
#include "pmx_launch.hpp"

using namespace pmx;

// The host-buffer pipeline of a batch whose buffers are page-locked: chunk i is uploaded on `stream`, computed on `stream2` behind the
// upload's event and downloaded on `stream3` behind the kernel's - the two copy directions have a stream (and a DMA engine) each, so chunk
// i + 1 goes up while chunk i - 1 comes down (with a stream per LANE, round 5, each lane's download stood in front of its next upload and
// the link carried one direction at a time: 61 GB/s for both together, profiles/r05/z_host_path.txt).  Pageable buffers: one chunk.
// A chunk is `cnt` rows: in_row bytes each up from `in` to d_in, `run` (a _dev entry) on them, out_row bytes each down from d_out to `out`.
// The permutation is the case where both sides are one buffer; a side whose rows are empty issues no copy.
template <class Run>
static int host_pipeline(pmx_ctx *ctx, size_t n, size_t step, const char *in, char *d_in, size_t in_row, char *out, char *d_out, size_t out_row,
                         Run &&run) {
    int rc = PMX_OK;
    size_t first = 0;
    for (int i = 0; first < n; first += step, ++i) {
        const size_t cnt = n - first < step ? n - first : step;
        const int slot = i % pmx_ctx::kPipeChunks;   // (at most kPipeChunks chunks: pipeline_rows)
        if (in_row) PMX_HIP(hipMemcpyAsync(d_in + first * in_row, in + first * in_row, cnt * in_row, hipMemcpyHostToDevice, ctx->stream));
        PMX_HIP(hipEventRecord(ctx->pipe_up[slot], ctx->stream));
        PMX_HIP(hipStreamWaitEvent(ctx->stream2, ctx->pipe_up[slot], 0));
        if ((rc = run(first, cnt, ctx->stream2))) return rc;
        PMX_HIP(hipEventRecord(ctx->pipe_done[slot], ctx->stream2));
        PMX_HIP(hipStreamWaitEvent(ctx->stream3, ctx->pipe_done[slot], 0));
        if (out_row) PMX_HIP(hipMemcpyAsync(out + first * out_row, d_out + first * out_row, cnt * out_row, hipMemcpyDeviceToHost, ctx->stream3));
    }
    PMX_HIP(hipStreamSynchronize(ctx->stream3));
    PMX_HIP(hipStreamSynchronize(ctx->stream2));
    PMX_HIP(hipStreamSynchronize(ctx->stream));
    return PMX_OK;
}

// chunks of a batch for the pinned pipeline: rows per chunk (a multiple of 256).  A chunk is a kernel launch of its own: at least 65536
// rows (below that a launch is bound by one permutation's latency, at t = 3 on the lone-permutation kernels), at most kPipeChunks chunks
// (2^20 t = 3 states: 16 chunks 2.50 ms, 8 chunks 2.56, 32 chunks 4.2 - profiles/r06/g_host_path_probe_graded_chunks_and_zero_copy_not_kept.txt)
static size_t pipeline_rows(size_t n) {
    size_t chunks = n >> 16;
    if (chunks <= 1) return n;
    if (chunks > (size_t)pmx_ctx::kPipeChunks) chunks = pmx_ctx::kPipeChunks;
    const size_t rows = (n + chunks - 1) / chunks;
    return (rows + 255) / 256 * 256;
}

// ---- permutation ---------------------------------------------------------------------------------
extern "C" int pmx_permute_batch_dev(pmx_ctx *ctx, uint64_t *d_states, size_t n, void *stream) {
    if (!ctx || (!d_states && n)) return set_error(PMX_ERR_ARG, "pmx_permute_batch_dev: null pointer");
    if (n == 0) return PMX_OK;
    if (int rc = dev_batch_args(d_states, nullptr, n)) return rc;
    PMX_BIND(ctx);
    PMX_HIP(launch_permute(ctx->dev, ctx->t, d_states, n, (hipStream_t)stream));
    return PMX_OK;
}

extern "C" int pmx_permute_batch(pmx_ctx *ctx, uint64_t *states, size_t n) {
    PMX_ABI_BEGIN("pmx_permute_batch")
    if (!ctx || (!states && n)) return set_error(PMX_ERR_ARG, "pmx_permute_batch: null pointer");
    if (n == 0) return PMX_OK;
    PMX_HOST_CALL(call, ctx);
    int rc = PMX_OK;
    const size_t row = (size_t)ctx->t * 32;
    size_t bytes = 0;
    if ((rc = batch_bytes(n, ctx->t, &bytes))) return rc;
    Staging layout;
    layout.add(n, row);   // the states [n][t][4]
    char *d = nullptr;
    if ((rc = call.stage(layout, &d))) return rc;
    const size_t step = call.pin(states, bytes) ? pipeline_rows(n) : n;   // pinned: upload / kernel / download overlap, both directions at once
    return host_pipeline(ctx, n, step, (const char *)states, d, row, (char *)states, d, row, [&](size_t first, size_t cnt, hipStream_t st) -> int {
        return pmx_permute_batch_dev(ctx, (uint64_t *)(d + first * row), cnt, st);
    });
    PMX_ABI_END
}

// ---- hash ----------------------------------------------------------------------------------------
extern "C" int pmx_hash_batch_dev(pmx_ctx *ctx, const uint64_t *d_in, size_t in_len, uint64_t *d_out, size_t out_len,
                                  size_t n, void *stream) {
    if (!ctx || (!d_in && n && in_len) || (!d_out && n && out_len)) return set_error(PMX_ERR_ARG, "pmx_hash_batch_dev: null pointer");
    if (n == 0) return PMX_OK;
    if (int rc = dev_batch_args(d_in, d_out, n)) return rc;
    PMX_BIND(ctx);
    // two elements in, one out, rate >= 2: this IS the 2-to-1 compression (same memory layout as one tree level), whose
    // launcher has the quad kernel for small batches - a batch of authentication paths advances one level per call
    if (in_len == 2 && out_len == 1 && ctx->dev.rounds.rate >= 2) {
        PMX_HIP(launch_compress(ctx->dev, ctx->t, d_in, d_out, n, (hipStream_t)stream));
        return PMX_OK;
    }
    PMX_HIP(launch_hash(ctx->dev, ctx->t, d_in, in_len, d_out, out_len, n, (hipStream_t)stream));
    return PMX_OK;
}

extern "C" int pmx_hash_batch(pmx_ctx *ctx, const uint64_t *in, size_t in_len, uint64_t *out, size_t out_len, size_t n) {
    PMX_ABI_BEGIN("pmx_hash_batch")
    if (!ctx || (!in && n && in_len) || (!out && n && out_len)) return set_error(PMX_ERR_ARG, "pmx_hash_batch: null pointer");
    if (n == 0) return PMX_OK;
    PMX_HOST_CALL(call, ctx);
    int rc = PMX_OK;
    size_t in_bytes = 0, out_bytes = 0;
    if ((rc = batch_bytes(n, in_len, &in_bytes)) || (rc = batch_bytes(n, out_len, &out_bytes))) return rc;
    const size_t in_row = in_len * 32, out_row = out_len * 32;
    Staging rows_in, rows_out;
    rows_in.add(n, in_row);     // the inputs [n][in_len][4]
    rows_out.add(n, out_row);   // the digests [n][out_len][4]
    char *d_in = nullptr, *d_out = nullptr;
    if ((rc = call.stage(rows_in, &d_in)) || (rc = call.stage(rows_out, &d_out))) return rc;
    const bool in_pinned = call.pin(in, in_bytes), out_pinned = call.pin(out, out_bytes, in_pinned);   // (a large `out` is registered either way)
    const size_t step = in_pinned && out_pinned ? pipeline_rows(n) : n;
    return host_pipeline(ctx, n, step, (const char *)in, d_in, in_row, (char *)out, d_out, out_row, [&](size_t first, size_t cnt, hipStream_t st) -> int {
        return pmx_hash_batch_dev(ctx, (const uint64_t *)(d_in + first * in_row), in_len, (uint64_t *)(d_out + first * out_row), out_len, cnt, st);
    });
    PMX_ABI_END
}
