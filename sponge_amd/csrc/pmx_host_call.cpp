// The call scope of the host-buffer entries (pmx_ctx.hpp: HostCall) and the argument checks the batch, sponge and matrix entries share.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/poseidon_mi355x.h"
#include "pmx_ctx.hpp"
#include "pmx_internal.hpp"

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
    if (PMX_HIP_CALL(hipHostRegister(const_cast<void *>(p), bytes, hipHostRegisterDefault)) != hipSuccess) {
        (void)hipGetLastError();
        (void)hip_injected();   // (absorbed: pmx_ctx.hpp)
        return false;
    }
    pins_[pinned_++].ptr = const_cast<void *>(p);
    return true;
}

// ---- the argument helpers several families share (pmx_ctx.hpp) ---------------------------------------
int pmx::batch_bytes(size_t n, size_t elems_per_row, size_t *bytes) {
    if (n > kMaxLaunchUnits) return set_error(PMX_ERR_ARG, "batch too large");
    if (elems_per_row && n > (SIZE_MAX / 32) / elems_per_row) return set_error(PMX_ERR_ARG, "batch byte size overflows size_t");
    *bytes = n * elems_per_row * 32;
    return PMX_OK;
}

int pmx::dev_batch_args(const void *a, const void *b, size_t n) {
    if (!aligned16(a) || !aligned16(b)) return set_error(PMX_ERR_ARG, "device pointers must be 16-byte aligned");
    if (n > kMaxLaunchUnits) return set_error(PMX_ERR_ARG, "batch too large");
    return PMX_OK;
}
