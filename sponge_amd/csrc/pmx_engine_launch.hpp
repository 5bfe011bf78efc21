// Launch<Engine>: the host side of the kernels of ONE engine instantiation (pmx_kernels.hpp), and its operation table
// (pmx_launch.hpp: EngineOps).  Naming engine_ops<Engine>() is what instantiates the engine's kernels in a translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "../../include/poseidon_mi355x.h"
#include "pmx_internal.hpp"
#include "pmx_kernels.hpp"
#include "pmx_launch.hpp"
#include "pmx_sponge_plan.hpp"

namespace pmx {

// ------------------------------------------------------------------------------------------------
// Launchers
// ------------------------------------------------------------------------------------------------
template <class Engine>
struct Launch {
    static int grid(size_t n) { return (int)((n + Engine::kUnits - 1) / Engine::kUnits); }
    // THE launch of an engine kernel, whichever: n units on `st` with the engine's workgroup and dynamic LDS; every kernel takes the config
    // and its constants first.  More than 64 KiB of dynamic LDS has to be asked for per kernel (and device).
    template <class K, class... A>
    static hipError_t enqueue(K kernel, const DevConfig &c, uint32_t t, size_t n, hipStream_t st, A... args) {
        const size_t lds = Engine::lds_bytes(c, t);
        if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel, dim3(grid(n)), dim3(Engine::kThreads), lds, st, c, c.consts, args...);
        return hipGetLastError();
    }

    static hipError_t permute(const DevConfig &c, uint32_t t, uint64_t *states, size_t n, hipStream_t st) {
        return enqueue(permute_kernel<Engine>, c, t, n, st, states, n);
    }
    static hipError_t hash(const DevConfig &c, uint32_t t, const uint64_t *in, size_t in_len, uint64_t *out,
                           size_t out_len, size_t n, hipStream_t st) {
        return enqueue(hash_kernel<Engine>, c, t, n, st, in, in_len, out, out_len, n);
    }
    static hipError_t hash_strided(const DevConfig &c, uint32_t t, const uint64_t *in, size_t in_len, size_t row_stride, size_t elem_stride,
                                   uint64_t *out, size_t out_len, size_t n, hipStream_t st) {
        return enqueue(hash_strided_kernel<Engine>, c, t, n, st, in, in_len, row_stride, elem_stride, out, out_len, n);
    }
    static hipError_t compress(const DevConfig &c, uint32_t t, const uint64_t *in, uint64_t *out, size_t n, hipStream_t st) {
        return enqueue(compress_kernel<Engine>, c, t, n, st, in, out, n);
    }
    static hipError_t compress_ary(const DevConfig &c, uint32_t t, const uint64_t *in, uint64_t *out, uint32_t arity, size_t n, hipStream_t st) {
        return enqueue(compress_ary_kernel<Engine>, c, t, n, st, in, arity, out, n);
    }
    static hipError_t compress_ary_bounded(const DevConfig &c, uint32_t t, const uint64_t *in, uint64_t *out, uint32_t arity, size_t n_children,
                                           size_t n, hipStream_t st) {
        return enqueue(compress_ary_bounded_kernel<Engine>, c, t, n, st, in, arity, n_children, out, n);
    }
    static hipError_t grind(const DevConfig &c, uint32_t t, const uint64_t *base, uint32_t index, uint32_t bits, uint64_t first, size_t n,
                            uint64_t *best, hipStream_t st) {
        return enqueue(grind_kernel<Engine>, c, t, n, st, base, index, bits, first, n, best);
    }
    // absorb / squeeze: per-lane kernels, or - on an engine whose permutation must stay wave-uniform - passes on its permutation
    // (pmx_sponge_plan.hpp).  Only the form the engine has is instantiated.
    template <class Rows>
    static hipError_t absorb_rows(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index, const uint64_t *in,
                                  const Rows &rows, size_t n, hipStream_t st, const PassScratch &scratch) {
        if constexpr (Engine::kWaveUniformOnly) {
            uint64_t *io = const_cast<uint64_t *>(in);   // (the absorb form of the pass kernels only reads `io`)
            return sponge_passes<false>(c, t, states, tag, index, io, rows, n, st, scratch);
        } else {
            return enqueue(absorb_kernel<Engine, Rows>, c, t, n, st, states, tag, index, in, rows, n);
        }
    }
    static hipError_t absorb(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index,
                             const uint64_t *in, size_t in_len, size_t n, hipStream_t st, const PassScratch &scratch) {
        return absorb_rows(c, t, states, tag, index, in, RowsFixed{in_len}, n, st, scratch);
    }
    static hipError_t absorb_varlen(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index, const uint64_t *in,
                                    const uint64_t *offsets, size_t max_len, size_t n, hipStream_t st, const PassScratch &scratch) {
        return absorb_rows(c, t, states, tag, index, in, RowsRagged{in, offsets, (uint32_t)max_len}, n, st, scratch);
    }
    static hipError_t squeeze(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index,
                              uint64_t *out, size_t out_len, size_t n, hipStream_t st, const PassScratch &scratch) {
        if constexpr (Engine::kWaveUniformOnly) {
            return sponge_passes<true>(c, t, states, tag, index, out, RowsFixed{out_len}, n, st, scratch);
        } else {
            return enqueue(squeeze_kernel<Engine>, c, t, n, st, states, tag, index, out, out_len, n);
        }
    }
    // the whole absorb / squeeze call as passes (pmx_sponge_plan.hpp): pass 0 over the batch, then one launch per further
    // permutation a sponge of the batch can need.  The two lists and the per-pass counters live in scratch the caller's
    // context keeps per stream (PassScratch).
    // (ragged rows, absorb only: `len` is the call's bound max_len, each sponge's walk ends at its own last pass)
    template <bool SQUEEZE, class Rows = RowsFixed>
    static hipError_t sponge_passes(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index, uint64_t *io,
                                    const Rows &rows, size_t n, hipStream_t st, const PassScratch &provider) {
        const size_t len = rows.bound();
        const size_t passes = SQUEEZE ? squeeze_passes(len, c.rounds.rate) : absorb_passes(len, c.rounds.rate);
        if (passes == 0 || n == 0) return hipSuccess;
        if (n > 0xffffffffull || len > kSpongeMaxLen) return hipErrorInvalidValue;
        const uint32_t last = (uint32_t)(passes - 1);    // (no sponge permutes in the last pass)
        const size_t launches = pass_launches(passes);
        PassLease lease(provider, st);                   // given back behind the last launch that reads the lists
        uint32_t *scratch = nullptr;                     // [counters, padded to 64 words | list A: n | list B: n]
        const size_t head = (passes + 63) / 64 * 64;
        hipError_t e = hipSuccess;
        uint32_t *lists[2] = {nullptr, nullptr};
        if (launches > 1) {                              // a second permutation is possible: its sponges travel on a list
            // (NOT hipMallocAsync / hipFreeAsync: with several contexts - several streams - alive, ROCm 7.0's stream-ordered pool
            // handed out blocks whose earlier use was still in flight; tools/soak.py lost sponges and took a memory fault that way)
            if (lease.take((head + 2 * n) * 4) != hipSuccess) return lease.err;
            scratch = lease.block;
            lists[0] = scratch + head;
            lists[1] = scratch + head + n;
            e = hipMemsetAsync(scratch, 0, head * 4, st);
        }
        // (named listed kernel first: the kernels of a code object lie in the order the source names them, and that order is kept)
        const auto listed = permute_listed_kernel<Engine, SQUEEZE, Rows>;
        const auto first = sponge_first_kernel<Engine, SQUEEZE, Rows>;
        if (e == hipSuccess) e = enqueue(first, c, t, n, st, states, tag, index, io, rows, n, last, lists[1], scratch ? scratch + 1 : nullptr);
        for (uint32_t p = 1; p < launches && e == hipSuccess; ++p)
            e = enqueue(listed, c, t, n, st, states, tag, index, io, rows, p, last, lists[p & 1], scratch + p, lists[(p + 1) & 1], scratch + p + 1);
        return e;
    }
    // what a launch of `op` would run on (pmx_ctx_engine_info): filled by the engine, completed per kernel family here
    static void describe(const DevConfig &c, uint32_t t, int op, size_t len, EngineInfo *o) {
        Engine::describe(*o);
        const bool driver = op == PMX_OP_ABSORB || op == PMX_OP_SQUEEZE;
        const bool passes = driver && Engine::kWaveUniformOnly;   // a pass is the permutation engine's launch
        o->waves_per_simd = driver && !passes ? Engine::kMinWavesDriver : Engine::kMinWaves;
        o->lds_bytes = (uint32_t)Engine::lds_bytes(c, t);
        o->launches = 1;
        if (passes) {
            const size_t passes_z = op == PMX_OP_SQUEEZE ? squeeze_passes(len, c.rounds.rate) : absorb_passes(len, c.rounds.rate);
            o->launches = (int)pass_launches(passes_z > 0x7fffffff ? 0x7fffffff : passes_z);
            std::snprintf(o->engine + std::strlen(o->engine), sizeof o->engine - std::strlen(o->engine), " x passes");
        }
    }
};

// the table of an engine instantiation (pmx_launch.hpp: EngineOps); taking the address of a launcher instantiates its kernels
template <class Engine>
static const EngineOps &engine_ops() {
    using L = Launch<Engine>;
    static constexpr EngineOps ops = {&L::permute, &L::hash, &L::hash_strided, &L::compress, &L::compress_ary, &L::compress_ary_bounded, &L::grind, &L::absorb, &L::absorb_varlen, &L::squeeze,
                                      &Engine::lds_bytes, &L::describe};
    return ops;
}

// ---- window engines: eight translation units (they dominate the build time, so they compile in parallel), the exponent (1, 3: alpha = 5;
// 2, 4: any other, ALPHA = 0) x the widths (1, 2: t = 3 .. 6; 3, 4: t = 7 .. 9), and 5 .. 8 the same four for a modulus that is 1 mod 2^29
// (HybridEngineP1).  Each exports the lookup of its own part:
template <int ALPHA, bool WIDE, bool P1>
const EngineOps *window_ops(uint32_t t);   // nullptr for a width the translation unit does not hold

}  // namespace pmx
