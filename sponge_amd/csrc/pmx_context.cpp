// C ABI of libposeidon_mi355x.so, the part that runs no kernel: the error text, contexts and their process-wide cache, pinned host and raw
// device memory.  See include/poseidon_mi355x.h for the contract and the reference interfaces each entry replaces.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
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
    // (a failure the test build made says so and names the call that was not made - it may lie below `what`, in the pass-scratch pool;
    // the wording is pmx_hooks.cpp's, the shipped library has none of it)
    if (const char *note = hip_injected()) return set_error(PMX_ERR_HIP, "%s: %s [%s]", what, hipGetErrorString(e), note);
    return set_error(PMX_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

}  // namespace pmx

using namespace pmx;

extern "C" int pmx_abi_version(void) { return PMX_ABI_VERSION; }

extern "C" const char *pmx_last_error(void) { return g_error; }

extern "C" int pmx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// the one teardown: of a whole context and, every member being tested, of one whose creation failed half way
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
    e = PMX_HIP_CALL(hipMalloc((void **)&ctx->d_consts, bytes));
    if (e == hipSuccess) e = PMX_HIP_CALL(hipMemcpy(ctx->d_consts, pp.consts.data(), bytes, hipMemcpyHostToDevice));
    if (e == hipSuccess) e = PMX_HIP_CALL(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    if (e == hipSuccess) e = PMX_HIP_CALL(hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    if (e == hipSuccess) e = PMX_HIP_CALL(hipStreamCreateWithFlags(&ctx->stream3, hipStreamNonBlocking));
    for (int i = 0; i < pmx_ctx::kPipeChunks && e == hipSuccess; ++i) {
        e = PMX_HIP_CALL(hipEventCreateWithFlags(&ctx->pipe_up[i], hipEventDisableTiming));
        if (e == hipSuccess) e = PMX_HIP_CALL(hipEventCreateWithFlags(&ctx->pipe_done[i], hipEventDisableTiming));
    }
    if (e != hipSuccess) {
        (void)ctx_free(ctx);   // (`e` is the first failure: whatever the teardown meets does not reach the text)
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

// Evicts idle contexts, oldest first, until `keep` of them are left: each is unlinked and remembered in `evicted`, which the caller has
// reserved room in (nothing may fail between unlinking a context and remembering it).  The caller holds the lock and frees them after
// letting go: stream synchronise + hipFree are not for under the lock.
static void cache_evict(CtxCache &cc, size_t keep, std::vector<pmx_ctx *> &evicted) {
    while (cc.idle.size() > keep) {
        pmx_ctx *old = cc.idle.front();
        cc.idle.pop_front();
        cache_unlink(cc, old);
        evicted.push_back(old);
    }
}

extern "C" int pmx_ctx_release(pmx_ctx *ctx) {
    PMX_ABI_BEGIN("pmx_ctx_release")
    if (!ctx) return PMX_OK;
    if (!ctx->cache_key) return set_error(PMX_ERR_ARG, "pmx_ctx_release: this context came from pmx_ctx_create; use pmx_ctx_destroy");
    CtxCache &cc = ctx_cache();
    std::vector<pmx_ctx *> evicted;
    evicted.reserve(2);
    {
        std::lock_guard<std::mutex> lock(cc.lock);
        if (ctx->cache_refs <= 0) return set_error(PMX_ERR_ARG, "pmx_ctx_release: released more often than acquired");
        if (--ctx->cache_refs == 0) {
            cc.idle.push_back(ctx);
            cache_evict(cc, kMaxIdle, evicted);
        }
    }
    for (pmx_ctx *old : evicted) (void)ctx_free(old);
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
        cache_evict(cc, 0, evicted);
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
// the preamble of the four raw entries: `body` runs with `device` checked and current
template <class Body>
static int on_device(int device, Body &&body) {
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return hip_fail(guard.err, "hipSetDevice");
    return body();
}

extern "C" int pmx_device_alloc(int device, void **d_ptr, size_t bytes) {
    if (!d_ptr) return set_error(PMX_ERR_ARG, "pmx_device_alloc: null pointer");
    *d_ptr = nullptr;
    return on_device(device, [&]() -> int {
        PMX_HIP(hipMalloc(d_ptr, bytes ? bytes : 16));
        return PMX_OK;
    });
}

extern "C" int pmx_device_free(int device, void *d_ptr) {
    if (!d_ptr) return PMX_OK;
    return on_device(device, [&]() -> int {
        PMX_HIP(hipFree(d_ptr));
        return PMX_OK;
    });
}

static int device_copy(int device, void *dst, const void *src, size_t bytes, void *stream, hipMemcpyKind kind) {
    if ((!dst || !src) && bytes) return set_error(PMX_ERR_ARG, "pmx_device_upload / download: null pointer");
    if (bytes == 0) return PMX_OK;
    return on_device(device, [&]() -> int {
        PMX_HIP(hipMemcpyAsync(dst, src, bytes, kind, (hipStream_t)stream));
        return PMX_OK;
    });
}

extern "C" int pmx_device_upload(int device, void *d_dst, const void *h_src, size_t bytes, void *stream) {
    return device_copy(device, d_dst, h_src, bytes, stream, hipMemcpyHostToDevice);
}

extern "C" int pmx_device_download(int device, void *h_dst, const void *d_src, size_t bytes, void *stream) {
    return device_copy(device, h_dst, d_src, bytes, stream, hipMemcpyDeviceToHost);
}

extern "C" int pmx_stream_synchronize(int device, void *stream) {
    return on_device(device, [&]() -> int {
        PMX_HIP(hipStreamSynchronize((hipStream_t)stream));
        return PMX_OK;
    });
}
