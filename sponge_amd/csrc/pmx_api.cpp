// C ABI of libposeidon_mi355x.so: contexts, validation, host<->device staging, kernel dispatch.
// See include/poseidon_mi355x.h for the contract and the reference interfaces each entry replaces.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/poseidon_mi355x.h"
#include "pmx_ctx.hpp"
#include "pmx_internal.hpp"
#include "pmx_prepare.hpp"
#include "pmx_launch.hpp"
#include "pmx_grind_plan.hpp"
#include "pmx_host_pieces.hpp"
#include "pmx_matrix_shape.hpp"
#include "pmx_sponge_plan.hpp"
#include "pmx_squeeze_cut.hpp"

namespace pmx {

static thread_local char g_error[512] = "";

int set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char *what) {
    return set_error(PMX_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

}  // namespace pmx

using namespace pmx;

// ---- the call scope (pmx_ctx.hpp) ---------------------------------------------------------------------
// Grow-only device staging: at least `bytes` bytes of ctx->scratch[slot].  Growing FREES the old block, which is why HostCall::stage
// hands a slot out once per call.
static int ctx_scratch(pmx_ctx *ctx, int slot, size_t bytes, void **out) {
    if (bytes == 0) bytes = 16;
    if (ctx->scratch_bytes[slot] < bytes) {
        void *old = ctx->scratch[slot];
        ctx->scratch[slot] = nullptr;
        ctx->scratch_bytes[slot] = 0;
        if (old) PMX_HIP(hipFree(old));
        PMX_HIP(hipMalloc(&ctx->scratch[slot], bytes));
        ctx->scratch_bytes[slot] = bytes;
    }
    *out = ctx->scratch[slot];
    return PMX_OK;
}

int HostCall::stage(const Staging &layout, char **base) {
    *base = nullptr;
    if (layout.overflowed()) return set_error(PMX_ERR_ARG, "batch byte size overflows size_t");
    if (slots_ == 4) return set_error(PMX_ERR_HOST, "a host-buffer call asked for a fifth staging block");
    void *d = nullptr;
    if (int rc = ctx_scratch(ctx, slots_, layout.bytes(), &d)) return rc;
    ++slots_;
    *base = (char *)d;
    return PMX_OK;
}

int HostCall::pinned_block(char **out) {
    if (!ctx->pinned) PMX_HIP(hipHostMalloc(&ctx->pinned, kSmallCallBytes, hipHostMallocDefault));
    *out = (char *)ctx->pinned;
    return PMX_OK;
}

static bool is_pinned(const void *p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();   // an ordinary (unregistered) host pointer: clear the sticky error
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

bool HostCall::pin(const void *p, size_t bytes, bool answer_wanted) {
    if (!p || bytes == 0) return true;
    if (!answer_wanted && bytes < ScopedPin::kMinBytes) return false;
    if (is_pinned(p)) return true;
    if (bytes < ScopedPin::kMinBytes || pinned_ == 2) return false;
    if (hipHostRegister(const_cast<void *>(p), bytes, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    pins_[pinned_++].ptr = const_cast<void *>(p);
    return true;
}

// The host-buffer pipeline of a batch whose buffers are page-locked: chunk i is uploaded on `stream`, computed on `stream2` behind the
// upload's event and downloaded on `stream3` behind the kernel's - the two copy directions have a stream (and a DMA engine) each, so chunk
// i + 1 goes up while chunk i - 1 comes down (with a stream per LANE, round 5, each lane's download stood in front of its next upload and
// the link carried one direction at a time: 61 GB/s for both together, profiles/r05/z_host_path.txt).  Pageable buffers: one chunk.
template <class Up, class Run, class Down>
static int host_pipeline(pmx_ctx *ctx, size_t n, size_t step, Up &&up, Run &&run, Down &&down) {
    int rc = PMX_OK;
    size_t first = 0;
    for (int i = 0; first < n; first += step, ++i) {
        const size_t cnt = n - first < step ? n - first : step;
        const int slot = i % pmx_ctx::kPipeChunks;   // (at most kPipeChunks chunks: pipeline_rows)
        if ((rc = up(first, cnt, ctx->stream))) return rc;
        PMX_HIP(hipEventRecord(ctx->pipe_up[slot], ctx->stream));
        PMX_HIP(hipStreamWaitEvent(ctx->stream2, ctx->pipe_up[slot], 0));
        if ((rc = run(first, cnt, ctx->stream2))) return rc;
        PMX_HIP(hipEventRecord(ctx->pipe_done[slot], ctx->stream2));
        PMX_HIP(hipStreamWaitEvent(ctx->stream3, ctx->pipe_done[slot], 0));
        if ((rc = down(first, cnt, ctx->stream3))) return rc;
    }
    PMX_HIP(hipStreamSynchronize(ctx->stream3));
    PMX_HIP(hipStreamSynchronize(ctx->stream2));
    PMX_HIP(hipStreamSynchronize(ctx->stream));
    return PMX_OK;
}

// n * elems_per_row * 32 bytes, or an error if that does not fit size_t / the launch grid
static int batch_bytes(size_t n, size_t elems_per_row, size_t *bytes) {
    if (n > (size_t)0x7fffffff * 64) return set_error(PMX_ERR_ARG, "batch too large");
    if (elems_per_row && n > (SIZE_MAX / 32) / elems_per_row) return set_error(PMX_ERR_ARG, "batch byte size overflows size_t");
    *bytes = n * elems_per_row * 32;
    return PMX_OK;
}

extern "C" int pmx_abi_version(void) { return PMX_ABI_VERSION; }

extern "C" const char *pmx_last_error(void) { return g_error; }

extern "C" int pmx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int pmx_ctx_create(const pmx_config *cfg, int device, pmx_ctx **out) {
    PMX_ABI_BEGIN("pmx_ctx_create")
    if (!cfg || !out) return set_error(PMX_ERR_ARG, "pmx_ctx_create: null pointer");
    *out = nullptr;
    if (!cfg->ark || !cfg->mds) return set_error(PMX_ERR_ARG, "pmx_ctx_create: null ark/mds");
    Prepared pp;
    std::string err;
    int rc = prepare(cfg, pp, err);   // the asserts of PoseidonConfig::new + limits of this build
    if (rc) return set_error(rc, "%s", err.c_str());
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return set_error(PMX_ERR_HIP, "no HIP device available (%s); this library has no CPU fallback", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return set_error(PMX_ERR_ARG, "device %d out of range [0,%d)", device, ndev);

    pmx_ctx *ctx = new (std::nothrow) pmx_ctx();
    if (!ctx) return set_error(PMX_ERR_HOST, "pmx_ctx_create: out of host memory");
    ctx->device = device;
    ctx->t = pp.t;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) { delete ctx; return hip_fail(guard.err, "hipSetDevice"); }

    const size_t bytes = pp.consts.size() * 4;
    e = hipMalloc((void **)&ctx->d_consts, bytes);
    if (e == hipSuccess) e = hipMemcpy(ctx->d_consts, pp.consts.data(), bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream3, hipStreamNonBlocking);
    for (int i = 0; i < pmx_ctx::kPipeChunks && e == hipSuccess; ++i) {
        e = hipEventCreateWithFlags(&ctx->pipe_up[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->pipe_done[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        for (hipStream_t st : {ctx->stream, ctx->stream2, ctx->stream3})
            if (st) (void)hipStreamDestroy(st);
        for (int i = 0; i < pmx_ctx::kPipeChunks; ++i) {
            if (ctx->pipe_up[i]) (void)hipEventDestroy(ctx->pipe_up[i]);
            if (ctx->pipe_done[i]) (void)hipEventDestroy(ctx->pipe_done[i]);
        }
        if (ctx->d_consts) (void)hipFree(ctx->d_consts);
        delete ctx;
        return hip_fail(e, "pmx_ctx_create: device setup");
    }
    DevConfig &d = ctx->dev;
    d.consts = ctx->d_consts;
    d.n_const_words = (uint32_t)pp.consts.size();
    d.mds_offset = (uint32_t)pp.mds_offset;
    d.opt_offset = (uint32_t)pp.opt_offset;
    d.coop_offset = (uint32_t)pp.coop_offset;
    d.mfma_offset = (uint32_t)pp.mfma_offset;
    d.mfma_dense = pp.mfma_dense ? 1u : 0u;
    d.win_offset = (uint32_t)pp.win_offset;
    d.io_offset = (uint32_t)pp.io_offset;
    d.has_opt = pp.has_opt ? 1u : 0u;
    {
        int lds = 0;
        if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess || lds <= 0) lds = 64 * 1024;
        d.max_lds_bytes = (uint32_t)lds;
    }
    d.rounds = pp.c;
    d.field = pp.f;
    d.field.io = nullptr;   // engines point it at consts + io_offset on the device
    d.one = pp.one;
    *out = ctx;
    return PMX_OK;
    PMX_ABI_END
}

static int ctx_free(pmx_ctx *ctx) {
    DeviceGuard guard(ctx->device);
    for (hipStream_t st : {ctx->stream, ctx->stream2, ctx->stream3}) {
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
    }
    for (int i = 0; i < pmx_ctx::kPipeChunks; ++i) {
        if (ctx->pipe_up[i]) (void)hipEventDestroy(ctx->pipe_up[i]);
        if (ctx->pipe_done[i]) (void)hipEventDestroy(ctx->pipe_done[i]);
    }
    for (int i = 0; i < 4; ++i)
        if (ctx->scratch[i]) (void)hipFree(ctx->scratch[i]);
    // (the caller's streams are the caller's to drain before it destroys the context, as with every *_dev call)
    for (pmx_ctx::PassBlock &b : ctx->pass_pool) {
        if (b.done) (void)hipEventDestroy(b.done);
        if (b.ptr) (void)hipFree(b.ptr);
    }
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->d_consts) (void)hipFree(ctx->d_consts);
    delete ctx;
    return PMX_OK;
}

extern "C" int pmx_ctx_destroy(pmx_ctx *ctx) {
    if (!ctx) return PMX_OK;
    if (ctx->cache_key) return set_error(PMX_ERR_ARG, "pmx_ctx_destroy: this context came from pmx_ctx_acquire; hand it back with pmx_ctx_release");
    return ctx_free(ctx);
}

// ---- shared contexts ---------------------------------------------------------------------------------
// CryptographicSponge::new clones the parameters into every sponge (src/poseidon/mod.rs:219-230) and downstream code
// calls it once per transcript.  Creating a device context per sponge would re-derive the sparse-round tables, allocate
// and upload every time, so the bindings take their context from this process-wide cache instead: one context per
// (config contents, device), reference-counted; idle contexts stay resident (at most kMaxIdle of them, oldest first
// out) so that  new -> drop -> new  does not rebuild either.
namespace {
struct CtxCache {
    std::mutex lock;
    std::unordered_map<uint64_t, std::vector<pmx_ctx *>> by_key;
    std::deque<pmx_ctx *> idle;   // refs == 0, oldest first
};
CtxCache &ctx_cache() {
    static CtxCache *c = new CtxCache();   // never destroyed: contexts may outlive static destructors' order
    return *c;
}
constexpr size_t kMaxIdle = 8;

std::string config_blob(const pmx_config *cfg, int device) {
    const size_t t = (size_t)cfg->rate + cfg->capacity, rounds = (size_t)cfg->full_rounds + cfg->partial_rounds;
    std::string b;
    auto put = [&](const void *p, size_t n) { b.append((const char *)p, n); };
    put(&device, sizeof device);
    put(&cfg->full_rounds, 4); put(&cfg->partial_rounds, 4); put(&cfg->alpha, 8); put(&cfg->rate, 4); put(&cfg->capacity, 4);
    put(cfg->modulus, 32);
    put(cfg->ark, rounds * t * 32);
    put(cfg->mds, t * t * 32);
    return b;
}
uint64_t fnv1a(const std::string &b) {
    uint64_t h = 1469598103934665603ull;
    for (unsigned char c : b) { h ^= c; h *= 1099511628211ull; }
    return h ? h : 1;
}
}  // namespace

// The cache lock is held only for the bookkeeping: a context is created (table derivation, hipMalloc, upload) and freed
// (stream synchronise, hipFree) outside it, so one thread building or evicting a context never stalls another thread's
// acquire or release.  Two threads that miss on the same new config both build one; the second to come back finds the
// first one's entry, takes a reference on it and frees its own.
static pmx_ctx *cache_find(CtxCache &cc, uint64_t key, const std::string &blob) {
    auto it = cc.by_key.find(key);
    if (it == cc.by_key.end()) return nullptr;
    for (pmx_ctx *c : it->second) {
        if (c->cache_blob == blob) {
            if (c->cache_refs++ == 0) {
                for (auto d = cc.idle.begin(); d != cc.idle.end(); ++d)
                    if (*d == c) { cc.idle.erase(d); break; }
            }
            return c;
        }
    }
    return nullptr;
}

extern "C" int pmx_ctx_acquire(const pmx_config *cfg, int device, pmx_ctx **out) {
    PMX_ABI_BEGIN("pmx_ctx_acquire")
    if (!cfg || !out) return set_error(PMX_ERR_ARG, "pmx_ctx_acquire: null pointer");
    *out = nullptr;
    if (!cfg->ark || !cfg->mds) return set_error(PMX_ERR_ARG, "pmx_ctx_acquire: null ark/mds");
    const uint64_t t64 = (uint64_t)cfg->rate + cfg->capacity, rounds = (uint64_t)cfg->full_rounds + cfg->partial_rounds;
    if (t64 == 0 || t64 > PMX_MAX_WIDTH || rounds == 0 || rounds > 4096) return pmx_ctx_create(cfg, device, out);   // let create() report it
    std::string blob = config_blob(cfg, device);
    const uint64_t key = fnv1a(blob);
    CtxCache &cc = ctx_cache();
    {
        std::lock_guard<std::mutex> lock(cc.lock);
        if (pmx_ctx *c = cache_find(cc, key, blob)) { *out = c; return PMX_OK; }
    }
    pmx_ctx *fresh = nullptr;
    int rc = pmx_ctx_create(cfg, device, &fresh);   // not under the lock
    if (rc) return rc;
    pmx_ctx *winner = nullptr;
    try {
        std::lock_guard<std::mutex> lock(cc.lock);
        winner = cache_find(cc, key, blob);
        if (!winner) {
            fresh->cache_blob = std::move(blob);
            try {
                cc.by_key[key].push_back(fresh);
            } catch (...) {
                // still under the lock: the map belongs to every thread (a bucket the failed insert may have left empty)
                auto it = cc.by_key.find(key);
                if (it != cc.by_key.end() && it->second.empty()) cc.by_key.erase(it);
                throw;
            }
            fresh->cache_key = key;      // set last: from here on the context belongs to the cache
            fresh->cache_refs = 1;
        }
    } catch (...) {
        (void)ctx_free(fresh);           // the lock is released by now; `fresh` never reached the cache
        throw;
    }
    if (winner) {
        (void)ctx_free(fresh);
        *out = winner;
    } else {
        *out = fresh;
    }
    return PMX_OK;
    PMX_ABI_END
}

// unlinks a context from its bucket (the caller holds the lock and frees it after letting go)
static void cache_unlink(CtxCache &cc, pmx_ctx *c) {
    auto b = cc.by_key.find(c->cache_key);
    if (b == cc.by_key.end()) return;
    for (auto it = b->second.begin(); it != b->second.end(); ++it)
        if (*it == c) { b->second.erase(it); break; }
    if (b->second.empty()) cc.by_key.erase(b);
}

extern "C" int pmx_ctx_release(pmx_ctx *ctx) {
    PMX_ABI_BEGIN("pmx_ctx_release")
    if (!ctx) return PMX_OK;
    if (!ctx->cache_key) return set_error(PMX_ERR_ARG, "pmx_ctx_release: this context came from pmx_ctx_create; use pmx_ctx_destroy");
    CtxCache &cc = ctx_cache();
    std::vector<pmx_ctx *> evicted;
    evicted.reserve(2);   // (nothing below may fail between unlinking a context and remembering it)
    {
        std::lock_guard<std::mutex> lock(cc.lock);
        if (ctx->cache_refs <= 0) return set_error(PMX_ERR_ARG, "pmx_ctx_release: released more often than acquired");
        if (--ctx->cache_refs == 0) {
            cc.idle.push_back(ctx);
            while (cc.idle.size() > kMaxIdle) {
                pmx_ctx *old = cc.idle.front();
                cc.idle.pop_front();
                cache_unlink(cc, old);
                evicted.push_back(old);
            }
        }
    }
    for (pmx_ctx *old : evicted) (void)ctx_free(old);   // stream synchronise + hipFree: not under the lock
    return PMX_OK;
    PMX_ABI_END
}

extern "C" int pmx_ctx_cache_clear(void) {
    PMX_ABI_BEGIN("pmx_ctx_cache_clear")
    CtxCache &cc = ctx_cache();
    std::vector<pmx_ctx *> evicted;
    {
        std::lock_guard<std::mutex> lock(cc.lock);
        evicted.reserve(cc.idle.size());
        while (!cc.idle.empty()) {
            pmx_ctx *old = cc.idle.front();
            cc.idle.pop_front();
            cache_unlink(cc, old);
            evicted.push_back(old);
        }
    }
    for (pmx_ctx *old : evicted) (void)ctx_free(old);
    return PMX_OK;
    PMX_ABI_END
}

extern "C" int pmx_ctx_width(const pmx_ctx *ctx) { return ctx ? (int)ctx->t : 0; }

extern "C" int pmx_ctx_engine_info(const pmx_ctx *ctx, int op, size_t n, size_t len, pmx_engine_info *out) {
    if (!ctx || !out) return set_error(PMX_ERR_ARG, "pmx_ctx_engine_info: null pointer");
    if (describe_launch(ctx->dev, ctx->t, op, n, len, out) != hipSuccess) return set_error(PMX_ERR_ARG, "pmx_ctx_engine_info: unknown op %d", op);
    return PMX_OK;
}

// the argument lines the batch *_dev entries share, in the order each of them tests them (a null pointer counts as aligned)
static int dev_batch_args(const void *a, const void *b, size_t n) {
    if (!aligned16(a) || !aligned16(b)) return set_error(PMX_ERR_ARG, "device pointers must be 16-byte aligned");
    if (n > (size_t)0x7fffffff * 64) return set_error(PMX_ERR_ARG, "batch too large");
    return PMX_OK;
}

// ---- pinned host memory ----------------------------------------------------------------------------
extern "C" int pmx_host_alloc(void **ptr, size_t bytes) {
    if (!ptr) return set_error(PMX_ERR_ARG, "pmx_host_alloc: null pointer");
    *ptr = nullptr;
    PMX_HIP(hipHostMalloc(ptr, bytes ? bytes : 16, hipHostMallocDefault));
    return PMX_OK;
}

extern "C" int pmx_host_free(void *ptr) {
    if (ptr) PMX_HIP(hipHostFree(ptr));
    return PMX_OK;
}

// ---- device memory for callers without HIP bindings ------------------------------------------------------
static int device_ok(int device) {
    const int ndev = pmx_device_count();
    if (ndev == 0) return set_error(PMX_ERR_HIP, "no HIP device available; this library has no CPU fallback");
    if (device < 0 || device >= ndev) return set_error(PMX_ERR_ARG, "device %d out of range [0,%d)", device, ndev);
    return PMX_OK;
}

extern "C" int pmx_device_alloc(int device, void **d_ptr, size_t bytes) {
    if (!d_ptr) return set_error(PMX_ERR_ARG, "pmx_device_alloc: null pointer");
    *d_ptr = nullptr;
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return hip_fail(guard.err, "hipSetDevice");
    PMX_HIP(hipMalloc(d_ptr, bytes ? bytes : 16));
    return PMX_OK;
}

extern "C" int pmx_device_free(int device, void *d_ptr) {
    if (!d_ptr) return PMX_OK;
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return hip_fail(guard.err, "hipSetDevice");
    PMX_HIP(hipFree(d_ptr));
    return PMX_OK;
}

static int device_copy(int device, void *dst, const void *src, size_t bytes, void *stream, hipMemcpyKind kind) {
    if ((!dst || !src) && bytes) return set_error(PMX_ERR_ARG, "pmx_device_upload / download: null pointer");
    if (bytes == 0) return PMX_OK;
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return hip_fail(guard.err, "hipSetDevice");
    PMX_HIP(hipMemcpyAsync(dst, src, bytes, kind, (hipStream_t)stream));
    return PMX_OK;
}

extern "C" int pmx_device_upload(int device, void *d_dst, const void *h_src, size_t bytes, void *stream) {
    return device_copy(device, d_dst, h_src, bytes, stream, hipMemcpyHostToDevice);
}

extern "C" int pmx_device_download(int device, void *h_dst, const void *d_src, size_t bytes, void *stream) {
    return device_copy(device, h_dst, d_src, bytes, stream, hipMemcpyDeviceToHost);
}

extern "C" int pmx_stream_synchronize(int device, void *stream) {
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return hip_fail(guard.err, "hipSetDevice");
    PMX_HIP(hipStreamSynchronize((hipStream_t)stream));
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
    return host_pipeline(
        ctx, n, step,
        [&](size_t first, size_t cnt, hipStream_t st) -> int {
            PMX_HIP(hipMemcpyAsync((char *)d + first * row, (char *)states + first * row, cnt * row, hipMemcpyHostToDevice, st));
            return PMX_OK;
        },
        [&](size_t first, size_t cnt, hipStream_t st) -> int { return pmx_permute_batch_dev(ctx, (uint64_t *)((char *)d + first * row), cnt, st); },
        [&](size_t first, size_t cnt, hipStream_t st) -> int {
            PMX_HIP(hipMemcpyAsync((char *)states + first * row, (char *)d + first * row, cnt * row, hipMemcpyDeviceToHost, st));
            return PMX_OK;
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
    return host_pipeline(
        ctx, n, step,
        [&](size_t first, size_t cnt, hipStream_t st) -> int {
            if (in_bytes) PMX_HIP(hipMemcpyAsync((char *)d_in + first * in_row, (const char *)in + first * in_row, cnt * in_row, hipMemcpyHostToDevice, st));
            return PMX_OK;
        },
        [&](size_t first, size_t cnt, hipStream_t st) -> int {
            return pmx_hash_batch_dev(ctx, (const uint64_t *)((char *)d_in + first * in_row), in_len, (uint64_t *)((char *)d_out + first * out_row), out_len, cnt, st);
        },
        [&](size_t first, size_t cnt, hipStream_t st) -> int {
            if (out_bytes) PMX_HIP(hipMemcpyAsync((char *)out + first * out_row, (char *)d_out + first * out_row, cnt * out_row, hipMemcpyDeviceToHost, st));
            return PMX_OK;
        });
    PMX_ABI_END
}

// ---- duplex sponge driver ------------------------------------------------------------------------
// The pass drivers launch one kernel per permutation a sponge of the call can need: a call is limited to kMaxPasses of them
// (pmx_host_pieces.hpp: 65536 rates of elements per sponge and call - 16 MiB at rate 8; longer inputs are absorbed in several calls,
// which is the same thing to a duplex sponge).
static int check_pass_count(const pmx_ctx *ctx, int op, size_t /*n*/, size_t len, const char *who) {
    const uint32_t rate = ctx->dev.rounds.rate;
    const size_t passes = rate == 0 ? 0 : (op == PMX_OP_SQUEEZE ? squeeze_passes(len, rate) : absorb_passes(len, rate));
    if (passes > kMaxPasses + 1)     // (passes - 1 permutation launches)
        return set_error(PMX_ERR_ARG, "%s: %zu elements per sponge is more than 65536 rates (%u) in one call; split the call", who, len, rate);
    return PMX_OK;
}

// PassScratch::get / done for a context (called with ctx->pass_lock held).  Nothing on this path frees memory (hipFree waits for
// the whole device) or asks a CALLER's stream anything (the handle may belong to a stream that is being captured, or that is gone):
// a block is released by the context's own event, recorded behind the last launch that uses it.
static hipError_t ctx_pass_scratch(void *owner, hipStream_t st, size_t bytes, uint32_t **out) {
    pmx_ctx *ctx = static_cast<pmx_ctx *>(owner);
    pmx_ctx::PassBlock *pick = nullptr;
    for (pmx_ctx::PassBlock &b : ctx->pass_pool)            // the block this stream used last: ordered behind that use by the stream itself
        if (b.recorded && b.stream == st && b.bytes >= bytes) { pick = &b; break; }
    if (!pick) {
        for (pmx_ctx::PassBlock &b : ctx->pass_pool) {      // the smallest idle block that is large enough
            // (!recorded: held by the call that is being enqueued - the ragged hash keeps its states in one while its passes take another)
            if (b.poisoned || !b.recorded || b.bytes < bytes || (pick && pick->bytes <= b.bytes)) continue;
            if (b.recorded && hipEventQuery(b.done) != hipSuccess) {
                (void)hipGetLastError();                    // not ready - or not queryable (recorded into a capture): not idle
                continue;
            }
            pick = &b;
        }
    }
    if (!pick) {
        pmx_ctx::PassBlock fresh;
        size_t want = (bytes + 4095) & ~(size_t)4095;
        for (const pmx_ctx::PassBlock &b : ctx->pass_pool)  // grow in doublings: an outgrown block stays in the pool for smaller calls
            if (b.bytes * 2 > want && b.bytes < bytes) want = b.bytes * 2;
        hipError_t e = hipMalloc(&fresh.ptr, want);
        if (e != hipSuccess) return e;
        e = hipEventCreateWithFlags(&fresh.done, hipEventDisableTiming);
        if (e != hipSuccess) {
            (void)hipFree(fresh.ptr);
            return e;
        }
        fresh.bytes = want;
        ctx->pass_pool.push_back(fresh);
        pick = &ctx->pass_pool.back();
    }
    pick->stream = st;
    pick->recorded = false;      // in use by a call that is being enqueued: `done` records the event
    *out = static_cast<uint32_t *>(pick->ptr);
    return hipSuccess;
}
static void ctx_pass_done(void *owner, hipStream_t st, uint32_t *block) {
    pmx_ctx *ctx = static_cast<pmx_ctx *>(owner);
    for (pmx_ctx::PassBlock &b : ctx->pass_pool) {
        if (b.ptr != block) continue;
        // a record that failed leaves `done` unrecorded (or holding an older, completed record): a query would call the block idle while
        // this call's launches may still read it - such a block is never handed to another stream again (its own stream orders the reuse)
        if (hipEventRecord(b.done, st) != hipSuccess) {
            (void)hipGetLastError();
            b.poisoned = true;
        }
        b.recorded = true;
        return;
    }
}
static PassScratch ctx_passes(pmx_ctx *ctx) { return PassScratch{ctx, ctx_pass_scratch, ctx_pass_done}; }

extern "C" int pmx_sponge_absorb_batch_dev(pmx_ctx *ctx, uint64_t *d_states, uint32_t *d_tag, uint32_t *d_index,
                                           const uint64_t *d_in, size_t in_len, size_t n, void *stream) {
    if (!ctx || ((!d_states || !d_tag || !d_index) && n) || (!d_in && n && in_len))
        return set_error(PMX_ERR_ARG, "pmx_sponge_absorb_batch_dev: null pointer");
    if (n == 0 || in_len == 0) return PMX_OK;  // absorbing an empty input changes nothing (mod.rs:234-236)
    if (int rc = dev_batch_args(d_states, d_in, n)) return rc;
    if (int rc = check_pass_count(ctx, PMX_OP_ABSORB, n, in_len, "pmx_sponge_absorb_batch_dev")) return rc;
    PMX_ABI_BEGIN("pmx_sponge_absorb_batch_dev")
    PMX_BIND(ctx);
    std::lock_guard<std::mutex> lock(ctx->pass_lock);
    PMX_HIP(launch_absorb(ctx->dev, ctx->t, d_states, d_tag, d_index, d_in, in_len, n, (hipStream_t)stream, ctx_passes(ctx)));
    return PMX_OK;
    PMX_ABI_END
}

extern "C" int pmx_sponge_squeeze_batch_dev(pmx_ctx *ctx, uint64_t *d_states, uint32_t *d_tag, uint32_t *d_index,
                                            uint64_t *d_out, size_t out_len, size_t n, void *stream) {
    if (!ctx || ((!d_states || !d_tag || !d_index) && n) || (!d_out && n && out_len))
        return set_error(PMX_ERR_ARG, "pmx_sponge_squeeze_batch_dev: null pointer");
    if (n == 0) return PMX_OK;
    if (int rc = dev_batch_args(d_states, d_out, n)) return rc;
    if (int rc = check_pass_count(ctx, PMX_OP_SQUEEZE, n, out_len, "pmx_sponge_squeeze_batch_dev")) return rc;
    PMX_ABI_BEGIN("pmx_sponge_squeeze_batch_dev")
    PMX_BIND(ctx);
    std::lock_guard<std::mutex> lock(ctx->pass_lock);
    PMX_HIP(launch_squeeze(ctx->dev, ctx->t, d_states, d_tag, d_index, d_out, out_len, n, (hipStream_t)stream, ctx_passes(ctx)));
    return PMX_OK;
    PMX_ABI_END
}

static int check_modes(const pmx_ctx *ctx, const uint32_t *tag, const uint32_t *index, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        if (tag[i] > PMX_MODE_SQUEEZING) return set_error(PMX_ERR_ARG, "sponge %zu: mode tag %u is neither Absorbing nor Squeezing", i, tag[i]);
        if (index[i] > ctx->dev.rounds.rate) return set_error(PMX_ERR_ARG, "sponge %zu: mode index %u > rate %u", i, index[i], ctx->dev.rounds.rate);
    }
    return PMX_OK;
}

// n sponges resident on the device for the length of a host-buffer call: [states | io | tag | index] in one staging block, where `io`
// is the data of a packed call (sponge_host) and empty otherwise.  The caller reads nothing back before its last piece is enqueued: a
// call that fails half way leaves the caller's sponges as they were.  (st_bytes: the caller's batch_bytes(n, t).)
struct ResidentSponges {
    Staging layout;
    size_t n, st_bytes, o_io, o_tag, o_index;
    char *d = nullptr;

    ResidentSponges(size_t n_, size_t st_bytes_, size_t io_bytes) : n(n_), st_bytes(st_bytes_) {
        layout.add(st_bytes, 1);
        o_io = layout.add(io_bytes, 1);
        o_tag = layout.add(n, 4);
        o_index = layout.add(n, 4);
        layout.add(0, 1);   // the block ends on a boundary: the packed call copies bytes() each way, the size it has always copied
    }
    int place(HostCall &call) { return call.stage(layout, &d); }
    uint64_t *states() const { return (uint64_t *)d; }
    uint64_t *io() const { return (uint64_t *)(d + o_io); }
    uint32_t *tag() const { return (uint32_t *)(d + o_tag); }
    uint32_t *index() const { return (uint32_t *)(d + o_index); }
    int upload(const uint64_t *h_states, const uint32_t *h_tag, const uint32_t *h_index, hipStream_t st) const {
        PMX_HIP(hipMemcpyAsync(states(), h_states, st_bytes, hipMemcpyHostToDevice, st));
        PMX_HIP(hipMemcpyAsync(tag(), h_tag, n * 4, hipMemcpyHostToDevice, st));
        PMX_HIP(hipMemcpyAsync(index(), h_index, n * 4, hipMemcpyHostToDevice, st));
        return PMX_OK;
    }
    int fresh(hipStream_t st) const {   // zero state, Absorbing{0} (mod.rs:219-230)
        PMX_HIP(hipMemsetAsync(d, 0, layout.bytes(), st));
        return PMX_OK;
    }
    int download(uint64_t *h_states, uint32_t *h_tag, uint32_t *h_index, hipStream_t st) const {
        PMX_HIP(hipMemcpyAsync(h_states, states(), st_bytes, hipMemcpyDeviceToHost, st));
        PMX_HIP(hipMemcpyAsync(h_tag, tag(), n * 4, hipMemcpyDeviceToHost, st));
        PMX_HIP(hipMemcpyAsync(h_index, index(), n * 4, hipMemcpyDeviceToHost, st));
        return PMX_OK;
    }
};

// `width` bytes of each of n rows between the caller's rows (of its pitch) and a packed [n][width] device block: a piece's columns.
// One row, or a piece as wide as the rows, is one contiguous copy.
static int copy_columns(void *dst, size_t dst_pitch, const void *src, size_t src_pitch, size_t width, size_t n, hipMemcpyKind kind,
                        hipStream_t st) {
    if (width == 0) return PMX_OK;
    if (n == 1 || (width == dst_pitch && width == src_pitch)) PMX_HIP(hipMemcpyAsync(dst, src, n * width, kind, st));
    else PMX_HIP(hipMemcpy2DAsync(dst, dst_pitch, src, src_pitch, width, n, kind, st));
    return PMX_OK;
}

// The resident walk of the host absorb and squeeze entries, in native elements: the sponges up once; every piece of fixed_piece
// (pmx_host_pieces.hpp; a call within kMaxPasses rates is its one piece) through `step`, a _dev entry on ctx->stream, with its columns
// moved up in front of it (`up`) or down behind it (`down`) between the caller's rows - `row` bytes each, of which a native element
// yields `unit`, the last one what is left - and a packed [n][width] block; the sponges down once.  An error half way through a call
// of several pieces leaves the caller's states and mode words untouched (a squeeze's `out` holds the pieces that were done).
template <class Step>
static int resident_walk(HostCall &call, uint64_t *states, uint32_t *tag, uint32_t *index, size_t n, size_t st_bytes, size_t elems, size_t unit,
                         size_t row, const char *up, char *down, Step &&step) {
    const size_t rate = call.ctx->dev.rounds.rate, max_elems = kMaxPasses * rate;
    ResidentSponges sp(n, st_bytes, 0);
    Staging columns;
    columns.add(n, std::min(row, max_elems * unit));   // the widest piece's columns
    char *d_io = nullptr;
    int rc = PMX_OK;
    if ((rc = sp.place(call)) || (rc = call.stage(columns, &d_io))) return rc;
    hipStream_t st = call.ctx->stream;
    if ((rc = sp.upload(states, tag, index, st))) return rc;
    size_t done = 0;   // elements per sponge so far
    do {
        const size_t piece = fixed_piece(done, elems, max_elems, rate);
        const size_t col = done * unit, width = std::min(row - col, piece * unit);
        if (up && (rc = copy_columns(d_io, width, up + col, row, width, n, hipMemcpyHostToDevice, st))) return rc;
        if ((rc = step(sp, d_io, piece, width, st))) return rc;
        if (down && (rc = copy_columns(down + col, row, d_io, width, width, n, hipMemcpyDeviceToHost, st))) return rc;
        done += piece;
    } while (done < elems);
    if ((rc = sp.download(states, tag, index, st))) return rc;
    PMX_HIP(hipStreamSynchronize(st));
    return PMX_OK;
}

// The host absorb and squeeze of field elements take any length, as the reference does (mod.rs:232-254, 321-341): a small call goes
// through the context's page-locked block, every other call is the resident walk.
static int sponge_host(pmx_ctx *ctx, uint64_t *states, uint32_t *tag, uint32_t *index, const uint64_t *in, uint64_t *out,
                       size_t len, size_t n, bool absorb) {
    PMX_ABI_BEGIN("pmx_sponge_*_batch")
    if (!ctx || ((!states || !tag || !index) && n)) return set_error(PMX_ERR_ARG, "pmx_sponge_*_batch: null pointer");
    if (n == 0) return PMX_OK;
    if (absorb && len == 0) return PMX_OK;
    if ((absorb && !in) || (!absorb && !out && len)) return set_error(PMX_ERR_ARG, "pmx_sponge_*_batch: null data pointer");
    int rc = check_modes(ctx, tag, index, n);
    if (rc) return rc;
    const size_t rate = ctx->dev.rounds.rate, max_len = kMaxPasses * rate;
    PMX_HOST_CALL(call, ctx);
    size_t st_bytes = 0, io_bytes = 0;   // (io: the widest piece)
    if ((rc = batch_bytes(n, ctx->t, &st_bytes)) || (rc = batch_bytes(n, std::min(len, max_len), &io_bytes))) return rc;
    auto step = [&](const ResidentSponges &sp, char *d_io, size_t piece, size_t, hipStream_t st) -> int {
        if (absorb) return pmx_sponge_absorb_batch_dev(ctx, sp.states(), sp.tag(), sp.index(), (const uint64_t *)d_io, piece, n, st);
        return pmx_sponge_squeeze_batch_dev(ctx, sp.states(), sp.tag(), sp.index(), (uint64_t *)d_io, piece, n, st);
    };
    // A handful of sponges (the single PoseidonSponge of the trait shims is n = 1): the call is all latency, and eight
    // separate copies from pageable memory cost as much as the permutation itself.  Pack [states | io | tag | index] into
    // the context's page-locked block: one copy in, the kernel, one copy out.  (One sponge's max_len elements are 2 MiB and more:
    // a call of several pieces never fits.)
    ResidentSponges sp(n, st_bytes, io_bytes);
    const size_t packed = sp.layout.bytes();
    if (!sp.layout.overflowed() && packed <= kSmallCallBytes) {
        char *h = nullptr;
        if ((rc = call.pinned_block(&h)) || (rc = sp.place(call))) return rc;
        std::memcpy(h, states, st_bytes);
        if (absorb) std::memcpy(h + sp.o_io, in, io_bytes);
        std::memcpy(h + sp.o_tag, tag, n * 4);
        std::memcpy(h + sp.o_index, index, n * 4);
        PMX_HIP(hipMemcpyAsync(sp.d, h, packed, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = step(sp, sp.d + sp.o_io, len, 0, ctx->stream))) return rc;
        PMX_HIP(hipMemcpyAsync(h, sp.d, packed, hipMemcpyDeviceToHost, ctx->stream));
        PMX_HIP(hipStreamSynchronize(ctx->stream));
        std::memcpy(states, h, st_bytes);
        std::memcpy(tag, h + sp.o_tag, n * 4);
        std::memcpy(index, h + sp.o_index, n * 4);
        if (!absorb && io_bytes) std::memcpy(out, h + sp.o_io, io_bytes);
        return PMX_OK;
    }
    return resident_walk(call, states, tag, index, n, st_bytes, len, 32, len * 32, (const char *)in, (char *)out, step);
    PMX_ABI_END
}

extern "C" int pmx_sponge_absorb_batch(pmx_ctx *ctx, uint64_t *states, uint32_t *mode_tag, uint32_t *mode_index,
                                       const uint64_t *in, size_t in_len, size_t n) {
    return sponge_host(ctx, states, mode_tag, mode_index, in, nullptr, in_len, n, true);
}

extern "C" int pmx_sponge_squeeze_batch(pmx_ctx *ctx, uint64_t *states, uint32_t *mode_tag, uint32_t *mode_index,
                                        uint64_t *out, size_t out_len, size_t n) {
    return sponge_host(ctx, states, mode_tag, mode_index, nullptr, out, out_len, n, false);
}

// ---- squeeze bytes and bits ------------------------------------------------------------------------
// squeeze_bytes / squeeze_bits (mod.rs:256-286): `len` output units (bytes, or bits stored a byte each) per sponge come from
// cut_elems(len, unit) native elements (pmx_squeeze_cut.hpp); to the pass limit and the engine choice the call is that native squeeze.
static int squeeze_cut_dev(pmx_ctx *ctx, uint64_t *d_states, uint32_t *d_tag, uint32_t *d_index, uint8_t *d_out, size_t len, size_t n,
                           void *stream, bool bits, const char *who) {
    if (!ctx || ((!d_states || !d_tag || !d_index) && n) || (!d_out && n && len)) return set_error(PMX_ERR_ARG, "%s: null pointer", who);
    if (n == 0) return PMX_OK;
    if (int rc = dev_batch_args(d_states, nullptr, n)) return rc;
    if (len && n > SIZE_MAX / len) return set_error(PMX_ERR_ARG, "batch byte size overflows size_t");
    const size_t elems = cut_elems(len, cut_unit(ctx->dev.field, bits));
    if (elems > kSpongeMaxLen) return set_error(PMX_ERR_ARG, "%s: %zu elements per sponge is too large", who, elems);   // (the plan's 32-bit arithmetic)
    if (int rc = check_pass_count(ctx, PMX_OP_SQUEEZE, n, elems, who)) return rc;
    size_t elem_bytes = 0;   // only its overflow check is wanted: the launcher indexes n * elems elements with size_t
    if (int rc = batch_bytes(n, elems, &elem_bytes)) return rc;
    PMX_ABI_BEGIN(who)
    PMX_BIND(ctx);
    std::lock_guard<std::mutex> lock(ctx->pass_lock);
    PMX_HIP(launch_squeeze_cut(ctx->dev, ctx->t, d_states, d_tag, d_index, d_out, len, bits, n, (hipStream_t)stream, ctx_passes(ctx)));
    return PMX_OK;
    PMX_ABI_END
}

extern "C" int pmx_sponge_squeeze_bytes_batch_dev(pmx_ctx *ctx, uint64_t *d_states, uint32_t *d_mode_tag, uint32_t *d_mode_index,
                                                  uint8_t *d_out, size_t num_bytes, size_t n, void *stream) {
    return squeeze_cut_dev(ctx, d_states, d_mode_tag, d_mode_index, d_out, num_bytes, n, stream, false, "pmx_sponge_squeeze_bytes_batch_dev");
}

extern "C" int pmx_sponge_squeeze_bits_batch_dev(pmx_ctx *ctx, uint64_t *d_states, uint32_t *d_mode_tag, uint32_t *d_mode_index,
                                                 uint8_t *d_out, size_t num_bits, size_t n, void *stream) {
    return squeeze_cut_dev(ctx, d_states, d_mode_tag, d_mode_index, d_out, num_bits, n, stream, true, "pmx_sponge_squeeze_bits_batch_dev");
}

// Host buffers: the resident walk, in native elements - a call beyond kMaxPasses rates of them is cut on element boundaries, the
// truncation falls into the last piece, and every piece's [n][width] block comes down into its columns of the caller's rows: n * len
// bytes over the link in all.
static int squeeze_cut_host(pmx_ctx *ctx, uint64_t *states, uint32_t *tag, uint32_t *index, uint8_t *out, size_t len, size_t n, bool bits,
                            const char *who) {
    PMX_ABI_BEGIN(who)
    if (!ctx || ((!states || !tag || !index) && n)) return set_error(PMX_ERR_ARG, "%s: null pointer", who);
    if (n == 0) return PMX_OK;
    if (!out && len) return set_error(PMX_ERR_ARG, "%s: null data pointer", who);
    // (the caller's `out`, n rows of len bytes, which the column copies index: not a staging size)
    if (len && n > SIZE_MAX / len) return set_error(PMX_ERR_ARG, "batch byte size overflows size_t");
    int rc = check_modes(ctx, tag, index, n);
    if (rc) return rc;
    const size_t unit = cut_unit(ctx->dev.field, bits), elems = cut_elems(len, (uint32_t)unit);
    size_t st_bytes = 0, piece_bytes = 0;
    if ((rc = batch_bytes(n, ctx->t, &st_bytes)) || (rc = batch_bytes(n, std::min(elems, kMaxPasses * ctx->dev.rounds.rate), &piece_bytes))) return rc;
    PMX_HOST_CALL(call, ctx);
    return resident_walk(call, states, tag, index, n, st_bytes, elems, unit, len, nullptr, (char *)out,
                         [&](const ResidentSponges &sp, char *d_io, size_t, size_t width, hipStream_t st) -> int {
                             return squeeze_cut_dev(ctx, sp.states(), sp.tag(), sp.index(), (uint8_t *)d_io, width, n, st, bits, who);
                         });
    PMX_ABI_END
}

extern "C" int pmx_sponge_squeeze_bytes_batch(pmx_ctx *ctx, uint64_t *states, uint32_t *mode_tag, uint32_t *mode_index, uint8_t *out,
                                              size_t num_bytes, size_t n) {
    return squeeze_cut_host(ctx, states, mode_tag, mode_index, out, num_bytes, n, false, "pmx_sponge_squeeze_bytes_batch");
}

extern "C" int pmx_sponge_squeeze_bits_batch(pmx_ctx *ctx, uint64_t *states, uint32_t *mode_tag, uint32_t *mode_index, uint8_t *out,
                                             size_t num_bits, size_t n) {
    return squeeze_cut_host(ctx, states, mode_tag, mode_index, out, num_bits, n, true, "pmx_sponge_squeeze_bits_batch");
}

// ---- proof-of-work grinding ------------------------------------------------------------------------
// The smallest nonce v of [first, first + count) with  c = sponge.clone(); c.absorb(&F::from(v)); c.squeeze_bits(bits) all false
// (mod.rs:232-254, 272-286): one state up, one word down, the candidates exist only in registers (pmx_kernels.hpp: grind_kernel).
// An Absorbing{rate} or Squeezing sponge permutes before it absorbs (mod.rs:239-252) whatever the nonce: that permutation runs once,
// on the copy of the state in the context's staging memory, and the search then absorbs at index 0.  The range is walked in chunks
// (pmx_grind_plan.hpp) of grind_chunk() candidates, the result words read back behind each.
extern "C" int pmx_sponge_grind(pmx_ctx *ctx, const uint64_t *state, uint32_t mode_tag, uint32_t mode_index, uint32_t bits, uint64_t first,
                                uint64_t count, uint64_t *nonce_out, int *found_out) {
    PMX_ABI_BEGIN("pmx_sponge_grind")
    if (!ctx || !state || !nonce_out || !found_out) return set_error(PMX_ERR_ARG, "pmx_sponge_grind: null pointer");
    int rc = check_modes(ctx, &mode_tag, &mode_index, 1);
    if (rc) return rc;
    const uint32_t modulus_bit_size = modulus_bits(ctx->dev.field);
    if (bits > modulus_bit_size - 1)
        return set_error(PMX_ERR_ARG, "pmx_sponge_grind: %u bits is more than one squeezed element yields (%u)", bits, modulus_bit_size - 1);
    if (!grind_range_ok(first, count)) return set_error(PMX_ERR_ARG, "pmx_sponge_grind: the nonce range ends beyond 2^64");
    *found_out = 0;
    if (count == 0) return PMX_OK;
    if (bits == 0) {   // squeeze_bits(0) is empty: every nonce is accepted
        *nonce_out = first;
        *found_out = 1;
        return PMX_OK;
    }
    PMX_HOST_CALL(call, ctx);
    // one copy up, 16 bytes down per chunk
    Staging layout;
    const size_t st_bytes = (size_t)ctx->t * 32;
    layout.add(ctx->t, 32);                       // the state
    const size_t o_res = layout.add(2, 8);        // the smallest accepted nonce | whether there is one
    char *h = nullptr, *d = nullptr;
    if ((rc = call.pinned_block(&h)) || (rc = call.stage(layout, &d))) return rc;
    uint64_t *h_res = (uint64_t *)(h + o_res), *d_state = (uint64_t *)d, *d_res = (uint64_t *)(d + o_res);
    std::memcpy(h, state, st_bytes);
    h_res[0] = UINT64_MAX;
    h_res[1] = 0;
    hipStream_t st = ctx->stream;
    PMX_HIP(hipMemcpyAsync(d, h, layout.bytes(), hipMemcpyHostToDevice, st));
    uint32_t index = mode_index;
    if (mode_tag == PMX_MODE_SQUEEZING || index == ctx->dev.rounds.rate) {   // mod.rs:241-244, 250: the same for every nonce
        PMX_HIP(launch_permute(ctx->dev, ctx->t, d_state, 1, st));
        index = 0;
    }
    const uint64_t chunk = grind_chunk(), chunks = grind_chunks(count, chunk);
    for (uint64_t k = 0; k < chunks; ++k) {
        const GrindChunk c = grind_chunk_at(first, count, chunk, k);
        PMX_HIP(launch_grind(ctx->dev, ctx->t, d_state, index, bits, c.first, (size_t)c.count, d_res, st));
        PMX_HIP(hipMemcpyAsync(h_res, d_res, 16, hipMemcpyDeviceToHost, st));
        PMX_HIP(hipStreamSynchronize(st));
        if (h_res[1]) {
            *nonce_out = h_res[0];
            *found_out = 1;
            break;
        }
    }
    return PMX_OK;
    PMX_ABI_END
}

// ---- variable-length rows ------------------------------------------------------------------------
// Row i of a call is in[offsets[i] .. offsets[i + 1]) (pmx_sponge_plan.hpp: varlen_row_len).  The _dev entries take the caller's bound
// max_len on every row: it sets the passes (check_pass_count) and clamps a longer row; device-resident offsets are not validated.
static int varlen_dev_args(const pmx_ctx *ctx, const void *d_states, const uint64_t *d_in, size_t max_len, size_t n, const char *who) {
    if (int rc = dev_batch_args(d_states, d_in, n)) return rc;
    if (n > 0xffffffffull) return set_error(PMX_ERR_ARG, "batch too large");
    if (max_len > kSpongeMaxLen) return set_error(PMX_ERR_ARG, "%s: max_len %zu is too large", who, max_len);
    return check_pass_count(ctx, PMX_OP_ABSORB, n, max_len, who);
}

extern "C" int pmx_sponge_absorb_varlen_batch_dev(pmx_ctx *ctx, uint64_t *d_states, uint32_t *d_tag, uint32_t *d_index, const uint64_t *d_in,
                                                  const uint64_t *d_offsets, size_t max_len, size_t n, void *stream) {
    if (!ctx || ((!d_states || !d_tag || !d_index || !d_offsets) && n) || (!d_in && n && max_len))
        return set_error(PMX_ERR_ARG, "pmx_sponge_absorb_varlen_batch_dev: null pointer");
    if (n == 0 || max_len == 0) return PMX_OK;   // every row is empty: nothing changes (mod.rs:234-236)
    if (int rc = varlen_dev_args(ctx, d_states, d_in, max_len, n, "pmx_sponge_absorb_varlen_batch_dev")) return rc;
    PMX_ABI_BEGIN("pmx_sponge_absorb_varlen_batch_dev")
    PMX_BIND(ctx);
    std::lock_guard<std::mutex> lock(ctx->pass_lock);
    PMX_HIP(launch_absorb_varlen(ctx->dev, ctx->t, d_states, d_tag, d_index, d_in, d_offsets, max_len, n, (hipStream_t)stream, ctx_passes(ctx)));
    return PMX_OK;
    PMX_ABI_END
}

extern "C" int pmx_hash_varlen_batch_dev(pmx_ctx *ctx, const uint64_t *d_in, const uint64_t *d_offsets, size_t max_len, uint64_t *d_out,
                                         size_t out_len, size_t n, void *stream) {
    if (!ctx || (!d_offsets && n) || (!d_in && n && max_len) || (!d_out && n && out_len))
        return set_error(PMX_ERR_ARG, "pmx_hash_varlen_batch_dev: null pointer");
    if (n == 0 || out_len == 0) return PMX_OK;   // nothing to write
    if (!aligned16(d_out)) return set_error(PMX_ERR_ARG, "device pointers must be 16-byte aligned");
    if (int rc = varlen_dev_args(ctx, nullptr, d_in, max_len, n, "pmx_hash_varlen_batch_dev")) return rc;
    if (int rc = check_pass_count(ctx, PMX_OP_SQUEEZE, n, out_len, "pmx_hash_varlen_batch_dev")) return rc;
    size_t st_bytes = 0;
    if (int rc = batch_bytes(n, ctx->t, &st_bytes)) return rc;
    PMX_ABI_BEGIN("pmx_hash_varlen_batch_dev")
    PMX_BIND(ctx);
    std::lock_guard<std::mutex> lock(ctx->pass_lock);
    PMX_HIP(launch_hash_varlen(ctx->dev, ctx->t, d_in, d_offsets, max_len, d_out, out_len, n, (hipStream_t)stream, ctx_passes(ctx)));
    return PMX_OK;
    PMX_ABI_END
}

// The host entries: offsets (and the mode words) are validated before anything is modified; only in[offsets[0] .. offsets[n]) is uploaded.
// A row longer than kMaxPasses rates is absorbed in pieces of at most that many elements (absorb(a ++ b) = absorb(a); absorb(b) to a duplex
// sponge, and the empty piece of a shorter row changes nothing); the states stay on the device between pieces.
static int varlen_host(pmx_ctx *ctx, uint64_t *states, uint32_t *tag, uint32_t *index, const uint64_t *in, const uint64_t *offsets,
                       bool hash, uint64_t *out, size_t out_len, size_t n, const char *who) {
    PMX_ABI_BEGIN(who)
    if (!ctx || (!offsets && n) || (!hash && (!states || !tag || !index) && n) || (hash && !out && n && out_len))
        return set_error(PMX_ERR_ARG, "%s: null pointer", who);
    if (n == 0 || (hash && out_len == 0)) return PMX_OK;
    for (size_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i])
            return set_error(PMX_ERR_ARG, "%s: row %zu: offsets decrease (%llu > %llu)", who, i, (unsigned long long)offsets[i],
                             (unsigned long long)offsets[i + 1]);
    const size_t total = offsets[n] - offsets[0];
    if (total && !in) return set_error(PMX_ERR_ARG, "%s: null input with %zu elements", who, total);
    int rc = PMX_OK;
    if (!hash && (rc = check_modes(ctx, tag, index, n))) return rc;
    if (total == 0 && !hash) return PMX_OK;   // every row empty: nothing changes (mod.rs:234-236)
    size_t longest = 0;
    for (size_t i = 0; i < n; ++i) longest = std::max<size_t>(longest, offsets[i + 1] - offsets[i]);
    const size_t piece = kMaxPasses * ctx->dev.rounds.rate, pieces = ragged_pieces(longest, piece);
    size_t st_bytes = 0, in_bytes = 0, out_bytes = 0;
    if ((rc = batch_bytes(n, ctx->t, &st_bytes)) || (rc = batch_bytes(total, 1, &in_bytes)) || (rc = batch_bytes(n, hash ? out_len : 0, &out_bytes)))
        return rc;
    if (hash && (rc = check_pass_count(ctx, PMX_OP_SQUEEZE, n, out_len, who))) return rc;
    std::vector<uint64_t> off(n + 1), packed;   // (in front of the scope: uploaded from until its drain)
    PMX_HOST_CALL(call, ctx);
    ResidentSponges sp(n, st_bytes, 0);
    Staging input, row_offsets, digests;
    input.add(pieces > 1 ? std::min(in_bytes, n * piece * 32) : in_bytes, 1);   // the input, or one piece of it
    row_offsets.add(n + 1, 8);
    digests.add(out_bytes, 1);
    char *d_in = nullptr, *d_off = nullptr, *d_out = nullptr;
    if ((rc = sp.place(call)) || (rc = call.stage(input, &d_in)) || (rc = call.stage(row_offsets, &d_off))) return rc;
    if (hash && (rc = call.stage(digests, &d_out))) return rc;
    hipStream_t st = ctx->stream;
    if ((rc = hash ? sp.fresh(st) : sp.upload(states, tag, index, st))) return rc;
    for (size_t k = 0; k < pieces; ++k) {
        // piece k of every row (ragged_range), rebased so that the uploaded input starts at offset 0
        const uint64_t *src = in + offsets[0] * 4;
        ragged_offsets(offsets, n, piece, k, off.data());
        if (pieces > 1) {
            packed.resize(off[n] * 4);
            for (size_t i = 0; i < n; ++i) {
                const size_t lo = ragged_range(offsets[i + 1] - offsets[i], piece, k).lo;
                if (off[i + 1] > off[i]) std::memcpy(packed.data() + off[i] * 4, in + (offsets[i] + lo) * 4, (off[i + 1] - off[i]) * 32);
            }
            src = packed.data();
        }
        if (off[n]) PMX_HIP(hipMemcpyAsync(d_in, src, off[n] * 32, hipMemcpyHostToDevice, st));
        PMX_HIP(hipMemcpyAsync(d_off, off.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
        if ((rc = pmx_sponge_absorb_varlen_batch_dev(ctx, sp.states(), sp.tag(), sp.index(), (const uint64_t *)d_in, (const uint64_t *)d_off,
                                                     std::min(longest, piece), n, st)))
            return rc;
        PMX_HIP(hipStreamSynchronize(st));   // (`off` and `packed` are rewritten for the next piece)
    }
    if (hash) {
        if ((rc = pmx_sponge_squeeze_batch_dev(ctx, sp.states(), sp.tag(), sp.index(), (uint64_t *)d_out, out_len, n, st))) return rc;
        PMX_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    } else if ((rc = sp.download(states, tag, index, st))) {
        return rc;
    }
    PMX_HIP(hipStreamSynchronize(st));
    return PMX_OK;
    PMX_ABI_END
}

extern "C" int pmx_sponge_absorb_varlen_batch(pmx_ctx *ctx, uint64_t *states, uint32_t *mode_tag, uint32_t *mode_index, const uint64_t *in,
                                              const uint64_t *offsets, size_t n) {
    return varlen_host(ctx, states, mode_tag, mode_index, in, offsets, false, nullptr, 0, n, "pmx_sponge_absorb_varlen_batch");
}

extern "C" int pmx_hash_varlen_batch(pmx_ctx *ctx, const uint64_t *in, const uint64_t *offsets, uint64_t *out, size_t out_len, size_t n) {
    return varlen_host(ctx, nullptr, nullptr, nullptr, in, offsets, true, out, out_len, n, "pmx_hash_varlen_batch");
}

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
    if (n_rows > (size_t)0x7fffffff * 64) return set_error(PMX_ERR_ARG, "batch too large");
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
    if (k > ((size_t)0x7fffffff * 64) / arity) return set_error(PMX_ERR_ARG, "batch byte size overflows size_t");
    return verify_host(ctx, nullptr, rows, row_len, indices, paths, depth, arity, (uint64_t)n_rows, false, k, root, ok_out);
    PMX_ABI_END
}
