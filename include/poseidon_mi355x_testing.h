/*
 * poseidon_mi355x_testing.h -- test hooks: of the device-group code (pmx_mgpu.cpp) of the grinding search's chunk size and of the matrix entries (pmx_hooks.cpp).  NOT part of the product ABI (poseidon_mi355x.h),
 * not in the Rust binding; the reference has no counterpart (it has no multi-device code at all,
 * src/poseidon/mod.rs:62-183).
 *
 * These symbols exist ONLY in libposeidon_mi355x_test.so: the shipped objects with pmx_mgpu.cpp and pmx_hooks.cpp compiled -DPMX_TEST_HOOKS
 * (sponge_amd/csrc/Makefile).  libposeidon_mi355x.so, the library that ships, neither exports them nor contains the state
 * they set (tests/test_abi_and_host.py checks both export tables).  State is process-wide and atomic.  The test build also
 * reads PMX_RCCL_LIBRARY=<path> when the first group is formed and binds THAT collective library (the tests' stand-in,
 * tests/fake_rccl, when the ranks of a rehearsal are separate processes); the shipped library binds RCCL by SONAME only.
 */
#ifndef POSEIDON_MI355X_TESTING_H
#define POSEIDON_MI355X_TESTING_H

#include "poseidon_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 (the test build is loaded). */
int pmx_test_hooks_enabled(void);

/* The host fan-out of pmx_mgpu_permute_batch / _hash_batch fails on local slot `fail_local` (-1: off) and, with
 * no_threads != 0, runs as if no worker thread could be started (the shards then go one after the other on the calling
 * thread). */
int pmx_mgpu_test_fault(int fail_local, int no_threads);

/* allow != 0: pmx_mgpu_create accepts the same HIP device in several slots (and up to PMX_MAX_LOCAL_DEVICES slots
 * whatever the number of visible devices); `devices` must then be given explicitly.  RCCL refuses two ranks on one
 * device, so this is only useful behind the stand-in collective library of tests/fake_rccl/, which lets every
 * world > 1 branch of the device-group code run on a one-GPU box. */
int pmx_mgpu_test_shared_device(int allow);

/* pmx_sponge_grind walks its nonce range in chunks of `candidates` per launch instead of the product's measured chunk (0: the product's
 * again).  For the test that needs a first hit in the THIRD chunk with an oracle leg of a few thousand permutations, and for the chunk
 * sweep of tools/grind_rate.py, which takes every size through the product's own host loop. */
int pmx_test_grind_chunk(uint64_t candidates);

/* pmx_matrix_leaves / pmx_matrix_commit upload their matrix in slabs of `rows` rows instead of what PMX_MATRIX_SLAB_BYTES holds (0: the
 * product's again), so that a matrix of a few hundred rows takes the multi-slab path - two buffers, the waits between the upload and
 * the compute stream, a short last slab - and the slab sweep of tools/matrix_commit_rate.py runs every size through the product's own
 * host loop. */
int pmx_test_matrix_slab_rows(uint64_t rows);

/* pmx_merkle_frontier_append and pmx_merkle_fixed walk their leaves in pieces of `leaves` leaves instead of the product's measured piece
 * (0: the product's again), so that an append of a thousand leaves takes the multi-piece path - the frontier handed from piece to piece on
 * the host - and the piece sweep of tools/merkle_fixed_rate.py runs every size through the product's own host loop. */
int pmx_test_merkle_fixed_piece(uint64_t leaves);

/* The strided hash kernel of the matrix entries on the caller's own device buffers: d_leaves [n_rows][4] receives
 * (new; absorb(row i); squeeze_native(1))[0] of the rows whose element k is at d_matrix + (i * row_stride + k * elem_stride) * 4 -
 * (row_len, 1) for a row-major matrix, (1, ld) for a column-major one of leading dimension ld.  It only enqueues on `stream`; both
 * pointers 16-byte aligned.  The product has no device-resident matrix entry; this one exists so that the kernel's memory footprint can be
 * laid into a guard-band arena (tests/arena.py) and its time taken between events. */
int pmx_test_matrix_leaves_dev(pmx_ctx *ctx, const uint64_t *d_matrix, size_t n_rows, size_t row_len, size_t row_stride, size_t elem_stride,
                               uint64_t *d_leaves, void *stream);

/* Injected HIP failures.  Every checked HIP call of the single-device entries (contexts, the host-buffer entries, the pass-scratch pool;
 * not the device groups, not the benchmark diagnostics) asks one function first.  The test build counts those calls per THREAD
 * (the state is thread_local, unlike the hooks above) and answers the armed one with hipErrorOutOfMemory in place of making it: the entry
 * leaves at once through its ordinary error path, PMX_ERR_HIP with "injected" and the call's expression text in pmx_last_error().  A
 * launcher of the kernel files is failed as a whole, through the checked call that wraps it.  Nothing reaches the device.
 * pmx_test_fail_hip: the calling thread's nth checked call from now fails (1-based), once; 0 disarms.  Either way the count starts again.
 * pmx_test_hip_calls: the checked calls of this thread since the last pmx_test_fail_hip.
 * pmx_test_hip_fired: the text "injected in place of <expression>" of the failure made since the last pmx_test_fail_hip, "" if none was:
 *   how a test finds a call whose failure the product absorbs (a registration that falls back, the event of a pool block). */
int pmx_test_fail_hip(int64_t nth);
int64_t pmx_test_hip_calls(void);
const char *pmx_test_hip_fired(void);

/* The pass-scratch pool of a context, read under its lock: the blocks it holds, those held by a call (taken and not given back - 0 between
 * calls, whichever way the last one ended) and those whose event could not be recorded, which no other stream is handed again. */
int pmx_test_pass_pool(pmx_ctx *ctx, size_t *blocks, size_t *held, size_t *poisoned);

#ifdef __cplusplus
}
#endif
#endif /* POSEIDON_MI355X_TESTING_H */
