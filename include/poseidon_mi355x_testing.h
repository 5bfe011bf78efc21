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

#ifdef __cplusplus
}
#endif
#endif /* POSEIDON_MI355X_TESTING_H */
