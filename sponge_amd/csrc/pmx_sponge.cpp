// C ABI of libposeidon_mi355x.so: the sponge family - the pass-scratch pool, absorb and squeeze of elements, bytes and bits, variable-length
// rows and the proof-of-work search, on device memory and on host buffers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/poseidon_mi355x.h"
#include "pmx_ctx.hpp"
#include "pmx_internal.hpp"
#include "pmx_launch.hpp"
#include "pmx_grind_plan.hpp"
#include "pmx_host_pieces.hpp"
#include "pmx_sponge_plan.hpp"
#include "pmx_squeeze_cut.hpp"

using namespace pmx;

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
        hipError_t e = PMX_HIP_CALL(hipMalloc(&fresh.ptr, want));
        if (e != hipSuccess) return e;
        e = PMX_HIP_CALL(hipEventCreateWithFlags(&fresh.done, hipEventDisableTiming));
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
        if (PMX_HIP_CALL(hipEventRecord(b.done, st)) != hipSuccess) {
            (void)hipGetLastError();
            (void)hip_injected();   // (absorbed: pmx_ctx.hpp)
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
// is the data of a packed call (sponge_host) and empty otherwise.  Nothing comes back into the caller's states and mode words before the
// call's last checked HIP call has succeeded (download / deliver): a call that fails - half way, or in its last synchronise - leaves the
// caller's sponges as they were.  (st_bytes: the caller's batch_bytes(n, t).)
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
    // The way back is two steps, so that no failure can leave the caller with states of one call and mode words of another: the whole block
    // down into the call's landing memory and the stream synchronised, which can fail; then host copies into the caller's arrays, which cannot.
    int download(HostCall &call, hipStream_t st) {
        h = call.landing(layout.bytes());
        PMX_HIP(hipMemcpyAsync(h, d, layout.bytes(), hipMemcpyDeviceToHost, st));
        PMX_HIP(hipStreamSynchronize(st));
        return PMX_OK;
    }
    void deliver(uint64_t *h_states, uint32_t *h_tag, uint32_t *h_index) const {
        std::memcpy(h_states, h, st_bytes);
        std::memcpy(h_tag, h + o_tag, n * 4);
        std::memcpy(h_index, h + o_index, n * 4);
    }
    char *h = nullptr;   // the landing memory of `download`
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
    if ((rc = sp.download(call, st))) return rc;
    sp.deliver(states, tag, index);
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
        PMX_HIP(hipStreamSynchronize(st));
        return PMX_OK;
    }
    if ((rc = sp.download(call, st))) return rc;
    sp.deliver(states, tag, index);
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
