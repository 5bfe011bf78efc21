// Private definition of pmx_ctx and the helpers shared by the entries of one device (pmx_context.cpp, pmx_host_call.cpp, pmx_batch.cpp,
// pmx_sponge.cpp, pmx_matrix.cpp), pmx_merkle.cpp (the trees) and pmx_mgpu.cpp (device groups).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/poseidon_mi355x.h"
#include "pmx_internal.hpp"
#include "pmx_staging.hpp"

struct pmx_ctx {
    int device = 0;
    uint32_t t = 0;
    pmx::DevConfig dev{};            // kernel-argument block (points at d_consts)
    uint32_t *d_consts = nullptr;    // device: constant table (pmx_prepare.hpp layout)
    hipStream_t stream = nullptr;    // used by the host-buffer entry points (and by a device group for this device)
    hipStream_t stream2 = nullptr;   // the pinned-memory pipeline: `stream` only uploads, `stream2` only computes, `stream3` only downloads
    hipStream_t stream3 = nullptr;
    static constexpr int kPipeChunks = 16;
    hipEvent_t pipe_up[kPipeChunks] = {}, pipe_done[kPipeChunks] = {};   // chunk i uploaded / computed (created with the context)
    void *scratch[4] = {nullptr, nullptr, nullptr, nullptr};   // grow-only device staging for the host-buffer entry points
    size_t scratch_bytes[4] = {0, 0, 0, 0};
    void *pinned = nullptr;          // page-locked host block for small host-buffer calls (allocated on first use)
    // The host-buffer entry points use the staging buffers and the two streams above: one caller at a time.  Contexts
    // handed out by pmx_ctx_acquire are shared between sponges (and threads), so those entry points take this lock;
    // the *_dev entry points only read the immutable fields and enqueue on the caller's stream.
    std::mutex host_lock;
    // Pass lists of the absorb / squeeze drivers that run as passes (pmx_engine_launch.hpp: sponge_passes): a pool of device blocks, each
    // with an event the CONTEXT owns, recorded on the caller's stream behind the last launch that uses the block.  A call takes the
    // block its stream used last (stream order makes that safe while the earlier call is still running), else any block whose event
    // has completed, else a new one; nothing is ever freed or queried through a caller's stream handle on the enqueue path - the
    // blocks go when the context goes.  pass_lock is held while a driver call enqueues, which also keeps two threads from
    // interleaving their launches on one stream of this context.
    struct PassBlock { void *ptr = nullptr; size_t bytes = 0; hipStream_t stream = nullptr; hipEvent_t done = nullptr; bool recorded = false; bool poisoned = false; };
    std::mutex pass_lock;
    std::vector<PassBlock> pass_pool;
    // pmx_ctx_acquire / pmx_ctx_release bookkeeping (0 for contexts made by pmx_ctx_create)
    uint64_t cache_key = 0;
    long cache_refs = 0;
    std::string cache_blob;          // the config bytes the key was computed from (collision check)
};

namespace pmx {

int hip_fail(hipError_t e, const char *what);

// The one door every checked HIP call of the single-device entries goes through, in front of the call (`what`: its expression text).
// Defined in pmx_hooks.cpp like grind_chunk() below: in the shipped library it returns hipSuccess and holds no state; the test build
// counts the calling thread's checked calls and, when pmx_test_fail_hip (include/poseidon_mi355x_testing.h) armed one, answers
// hipErrorOutOfMemory in its place - the call itself is then NOT made, and the entry leaves through its ordinary error path.
hipError_t hip_inject(const char *what);
// The wording of the calling thread's injected failure, once: hip_fail asks it for the message, and so does a site that absorbs the
// failure of its call, so that it cannot word a later one.  Null otherwise, and always in the shipped library.
const char *hip_injected();

// a checked call as an expression, for the sites that look at the status themselves
#define PMX_HIP_CALL(expr) (::pmx::hip_inject(#expr) == hipSuccess ? (expr) : hipErrorOutOfMemory)

#define PMX_HIP(expr)                                             \
    do {                                                          \
        hipError_t e_ = PMX_HIP_CALL(expr);                       \
        if (e_ != hipSuccess) return ::pmx::hip_fail(e_, #expr);  \
    } while (0)

// Every entry point runs with its context's device current and puts the caller's device back on the way out: in a
// process that drives several GPUs (torch, a device group) a call must not leave the thread's current device changed
// behind the caller's back.
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) err = hipSetDevice(device);
        else prev = -1;   // nothing to restore
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// Candidates per launch of pmx_sponge_grind (pmx_sponge.cpp).  Defined in pmx_hooks.cpp, the object that exists in a shipped and a test
// build: the measured constant in the shipped library; the test build lets pmx_test_grind_chunk (include/poseidon_mi355x_testing.h)
// replace it, so that a test can put a hit into the third chunk without an oracle leg of two product chunks, and the chunk sweep can
// take every size through the product's own host loop.
uint64_t grind_chunk();
// Rows per upload slab of the matrix entries (pmx_matrix.cpp), the same way: 0 in the shipped library - the slab is then what
// PMX_MATRIX_SLAB_BYTES of device memory holds (pmx_matrix_shape.hpp: matrix_slab_rows) - or what pmx_test_matrix_slab_rows set, so that
// a matrix of a few hundred rows takes the multi-slab path and the slab sweep runs every size through the product's own host loop.
uint64_t matrix_slab_rows_hook();
// Leaves per piece of pmx_merkle_frontier_append and pmx_merkle_fixed (pmx_merkle.cpp), the same way: the constant of pmx_hooks.cpp in
// the shipped library, or what pmx_test_merkle_fixed_piece set, so that an append of a thousand leaves takes the multi-piece path and the
// piece sweep of tools/merkle_fixed_rate.py runs every size through the product's own host loop.
uint64_t merkle_fixed_piece();

#define PMX_BIND(ctx)                                                                \
    ::pmx::DeviceGuard device_guard_((ctx)->device);                                 \
    if (device_guard_.err != hipSuccess) return ::pmx::hip_fail(device_guard_.err, "hipSetDevice")

// Host-buffer entry points queue asynchronous copies that read and write the CALLER's memory: whatever way they
// leave (including an error half way through), nothing may still be in flight on the context's streams.
struct StreamDrain {
    pmx_ctx *ctx;
    ~StreamDrain() {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(ctx->stream2);
        (void)hipStreamSynchronize(ctx->stream3);
    }
};

// A pageable buffer of a large call is page-locked for the length of the call (hipHostRegister: 4.2 ms for the 96 MiB of 2^20 t = 3
// states, unregister 0.1 ms - profiles/r06/g_host_path_probe.txt) so that it takes the pinned pipeline: 7 ms instead of the 8 ... 20 ms of
// the runtime's own staging through bounce buffers.
struct ScopedPin {
    void *ptr = nullptr;
    ~ScopedPin() {
        if (ptr && hipHostUnregister(ptr) != hipSuccess) (void)hipGetLastError();
    }
    static constexpr size_t kMinBytes = (size_t)16 << 20;   // below this the registration costs more than it saves
};

// What a host-buffer call of at most this many bytes stages through: the context's page-locked block, one copy each way.
constexpr size_t kSmallCallBytes = 64 * 1024;

// The scope of one host-buffer call (pmx_host_call.cpp has the bodies): made at the top of the entry's body with PMX_HOST_CALL, handed to the
// helpers that stage for it.  It binds the context's device, holds host_lock and drains the context's streams on the way out.  The
// MEMBER ORDER is the order of the call's end: the streams are drained first, then the caller's buffers are unregistered, then the
// lock goes and the caller's device comes back.
class HostCall {
public:
    explicit HostCall(pmx_ctx *c) : ctx(c), guard_(c->device), lock_(c->host_lock), drain_{c} {}
    HostCall(const HostCall &) = delete;
    HostCall &operator=(const HostCall &) = delete;
    hipError_t bind_error() const { return guard_.err; }

    // The next of the context's four grow-only device blocks, at least layout.bytes() long, 16-byte aligned: a block is taken once per
    // call (asking twice could free what the first asker still holds), so a layout states everything its block carries.  An overflowed
    // layout and a fifth block are errors.
    int stage(const Staging &layout, char **base);
    // the context's page-locked block of kSmallCallBytes, allocated on first use
    int pinned_block(char **out);
    // Whether copies from / to [p, p + bytes) may take the chunked pipeline: the buffer was page-locked on entry, or - from
    // ScopedPin::kMinBytes on - this call has registered it, until the streams are drained.  A registration that fails (locked-memory
    // limit, a range that is not plain memory) leaves the buffer as it is: false.  An empty buffer holds nothing back.  A caller whose
    // path does not hang on the answer says so: a buffer too small to register is then not even asked about.
    bool pin(const void *p, size_t bytes, bool answer_wanted = true);
    // `bytes` of host memory that live until the streams are drained: where an inout buffer of the caller comes down, to be copied into
    // the caller's memory only once the call can no longer fail.  One per call; std::bad_alloc is the entry's catch-all's.
    char *landing(size_t bytes) {
        landing_.resize(bytes);
        return landing_.data();
    }

    pmx_ctx *const ctx;

private:
    DeviceGuard guard_;
    std::lock_guard<std::mutex> lock_;
    ScopedPin pins_[2];
    std::vector<char> landing_;   // (freed behind the drain: downloads may be in flight into it)
    StreamDrain drain_;
    int slots_ = 0, pinned_ = 0;
};

#define PMX_HOST_CALL(call, ctx)                                                     \
    ::pmx::HostCall call(ctx);                                                       \
    if (call.bind_error() != hipSuccess) return ::pmx::hip_fail(call.bind_error(), "hipSetDevice")

// One staged verify body behind pmx_merkle_verify_paths, its arity-k and ragged variants and pmx_matrix_verify_rows (pmx_merkle.cpp).
// The matrix entry has no leaves: it passes its k opened rows [k][row_len][4], which ride in front of `ok` and are hashed into the leaves.
int verify_host(pmx_ctx *ctx, const uint64_t *leaves, const uint64_t *rows, size_t row_len, const uint64_t *indices, const uint64_t *paths,
                size_t depth, uint32_t arity, uint64_t limit, bool pairs, size_t k, const uint64_t *root, uint8_t *ok_out);

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// The launch-grid bound: the most units (states, rows, sponges, compressions) an entry hands to one launch, a grid of 2^31 - 1
// workgroups of 64 units.  What the entries test behind "batch too large".
constexpr size_t kMaxLaunchUnits = (size_t)0x7fffffff * 64;
// The argument helpers the batch, sponge and matrix entries share (pmx_host_call.cpp):
// n * elems_per_row * 32 bytes, or an error if that does not fit size_t / the launch grid
int batch_bytes(size_t n, size_t elems_per_row, size_t *bytes);
// the argument lines the batch *_dev entries share, in the order each of them tests them (a null pointer counts as aligned)
int dev_batch_args(const void *a, const void *b, size_t n);

}  // namespace pmx
