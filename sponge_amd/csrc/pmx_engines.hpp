// gfx950 engines of the batched Poseidon permutation and duplex-sponge driver.  Their kernels: pmx_kernels.hpp; the launchers of an
// engine instantiation: pmx_engine_launch.hpp; the translation units that instantiate them: pmx_device.hip (the quad and the
// run-time-width engine, the engine choice and the public launchers) and pmx_device_window.hip (the window engines).
//
// Work decomposition: one lane owns one sponge state; a wavefront owns 64 contiguous states of the
// [n][t][4]u64 batch.  State I/O goes through LDS so that every global access is a full-width
// 16-B-per-lane contiguous stream, whatever t is.  Round constants and the MDS matrix are wave-uniform.
// Arithmetic: pmx_field.hpp (unsaturated 9 x 29-bit Montgomery form); round schedule: pmx_permute.hpp.
//
// Engines (same interface: unit / owns / writes_mode, load_states / store_states / get / set / zero / permute), one per regime:
//   QuadEngine<ALPHA>          t = 3, launches of <= 32768 units (latency-bound: narrow tree levels, a handful of sponges):
//                              one state per quad of lanes, sparse rounds three multiplications deep.
//   HybridEngine<T, ALPHA>     t = 3..9 on the optimised schedule: state in VGPRs, the element loop of the full rounds' S-boxes rolled
//                              through one LDS scratch array per wave, EVERY product by a constant a layer on the matrix cores
//                              (pmx_mfma.hpp: the dense layers, and the partial rounds as windows closed by one layer each).
//   LdsEngine<ALPHA>           any width at run time (t = 2, 10..16, no partial section, a zero in the schedule's algebra): the
//                              reference's dense schedule, state kept in LDS as [element][limb][lane], element loops rolled.
// All three run the same permute / hash / compress / absorb / squeeze kernels; the hybrid engines run absorb / squeeze as passes.
//
// Reference semantics implemented here (file:line in /root/reference):
//   permute        src/poseidon/mod.rs:95-118   (apply_ark :76-80, apply_s_box :63-74, apply_mds :82-93)
//   absorb         src/poseidon/mod.rs:232-254 + absorb_internal :121-150
//   squeeze        src/poseidon/mod.rs:321-341 + squeeze_internal :153-182
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>

#include "pmx_field.hpp"
#include "pmx_internal.hpp"
#include "pmx_launch.hpp"
#include "pmx_permute.hpp"

namespace pmx {

extern __shared__ uint4 pmx_lds[];  // dynamic LDS, 16-byte granules

// Where a unit of a call (a state, a hash row, a compression, a sponge) lives, for the engines that give every lane one unit
// (HybridEngine, LdsEngine): unit = the global lane index; the lane holds, and so stores, every element of its state and
// writes its sponge's mode words.  QuadEngine answers the same questions for four lanes per unit.
template <int THREADS>
struct LanePerUnit {
    static constexpr int kThreads = THREADS, kUnits = THREADS;   // lanes / units per workgroup
    __device__ __forceinline__ static size_t unit() { return (size_t)blockIdx.x * THREADS + threadIdx.x; }
    __device__ __forceinline__ static constexpr bool owns(uint32_t /*i*/) { return true; }
    __device__ __forceinline__ static constexpr bool writes_mode() { return true; }
};

// ------------------------------------------------------------------------------------------------
// HybridEngine: t = 3..9 on the optimised schedule, every product by a constant on the matrix cores (pmx_mfma.hpp): the dense layers
// and, as windows of t S-boxes per layer, the linear part of the partial rounds.  State in registers (9 t VGPRs); every wave has one
// LDS scratch array [element][limb][lane] (2.25 (t - 1) KiB) that gives the rolled S-box loop of the full rounds and the layers' output
// rows their dynamic indexing (pmx_permute.hpp: permute_hybrid) and doubles as the staging area of the coalesced ABI store.
// Wave-uniform kernels only (permute, hash, compress, and the passes of the absorb / squeeze driver, which ARE permutation launches:
// inside a per-lane loop not every lane is active, and the lane exchange of the rows needs both lanes of a pair).
// (Rounds 1-4 also had this engine with VALU rows and sparse partial rounds, and a register engine for t = 3; since round 6 every config
// that has the optimised schedule has the window tables - any modulus - and the rest runs on the run-time-width engine.)
// ------------------------------------------------------------------------------------------------
// Register bounds (their byte strings and sums want registers), measured per width:
#ifndef PMX_MFMA_4WAVE_MAX_T
#define PMX_MFMA_4WAVE_MAX_T 3   // (t = 3: 120 VGPRs - four waves per SIMD without a spill)
#endif
#ifndef PMX_MFMA_3WAVE_MAX_T
#define PMX_MFMA_3WAVE_MAX_T 5
#endif
// Four waves per workgroup (one per SIMD), two workgroups per CU at t = 9 (8 x 18 KiB of scratch).  Since round 6 the rows' tables are
// streamed by every wave for itself (pmx_mfma.hpp: no LDS tile, no workgroup barrier inside the permutation); the workgroup only shares
// the barriers of the state store staging.  (One wave per workgroup was measured: +-0, profiles/r06/b_ab_*.)
constexpr int kMfmaWaves = 4;
template <int T, int ALPHA>
struct HybridEngine : LanePerUnit<64 * kMfmaWaves> {
    static_assert(T >= PMX_MFMA_MIN_T && T <= PMX_MFMA_MAX_T && mfma_window_for(T) > 0, "the window engines cover t = 3 .. 9");
    static constexpr int kWaves = kMfmaWaves;
    // waves per SIMD the register allocation must allow (4: <= 128 VGPRs, 3: <= 168, 2: <= 256)
    static constexpr int kMinWaves = T <= PMX_MFMA_4WAVE_MAX_T ? 4 : T <= PMX_MFMA_3WAVE_MAX_T ? 3 : 2;
    static constexpr int kMinWavesDriver = 2;   // (the pass kernels carry the driver's walk around the permutation: held to two waves)
    // the rows exchange operands between the lanes of a pair (l, l + 32): permute() must be reached by every lane of the wave - never
    // from a per-lane loop (absorb_kernel / squeeze_kernel static_assert on this; the drivers run as passes, sponge_first_kernel)
    static constexpr bool kWaveUniformOnly = true;
    static constexpr int kChunks = 2 * T;
    // one wave's LDS region: scratch slots for elements 0..T-2 (2304 B each) or the ABI staging of its 64 states
    // (2048 T B), whichever is larger
    static constexpr size_t kScratchBytes = (size_t)(T - 1) * kN * 64 * 4, kStageBytes = (size_t)64 * kChunks * 16;
    static constexpr size_t kWaveBytes = kScratchBytes > kStageBytes ? kScratchBytes : kStageBytes;

    struct Scratch {
        uint32_t *base;   // + lane
        __device__ __forceinline__ Fe get(uint32_t i) const {
            Fe r;
#pragma unroll
            for (int w = 0; w < kN; ++w) r.l[w] = base[(i * kN + w) * 64];
            return r;
        }
        __device__ __forceinline__ void set(uint32_t i, const Fe &v) {
#pragma unroll
            for (int w = 0; w < kN; ++w) base[(i * kN + w) * 64] = v.l[w];
        }
    };

    Fe s[T];
    Rounds c;
    FieldRt f;
    Fe one;
    OptTables tb;
    Scratch sc;
    uint4 *region;    // this wave's LDS region
    uint32_t lane;

    static size_t lds_bytes(const DevConfig & /*d*/, uint32_t /*t*/) { return kWaves * kWaveBytes; }

    __device__ __forceinline__ HybridEngine(const DevConfig &d, const uint32_t *consts) : c(d.rounds), f(d.field), one(d.one) {
        f.io = consts + d.io_offset;
        tb.ark = consts + d.opt_offset;
        tb.mfma = consts + d.mfma_offset;
        tb.win = consts + d.win_offset;
        lane = threadIdx.x & 63;
        region = pmx_lds + (threadIdx.x >> 6) * (kWaveBytes / 16);
        sc.base = reinterpret_cast<uint32_t *>(region) + lane;
    }

    __device__ __forceinline__ void zero() {
        static_for<0, T>([&](auto i) { s[i] = fe_zero(); });
    }
    __device__ __forceinline__ Fe from_abi(const Abi &x) const { return fe_from_abi_scaled(x); }      // the optimised schedule carries the ABI residue as its internal form (pmx_field.hpp: fe_from_abi_scaled)
    __device__ __forceinline__ Abi to_abi(const Fe &x) const { return fe_to_abi_scaled(x, f); }

    // widths whose permute kernel otherwise keeps spills inside the rounds read their elements in a rolled loop (t = 6 at three waves per
    // SIMD: 76 -> 12 bytes of scratch; t = 9: 76 -> 0); t = 7, 8 have none and lose 1 %
    static constexpr bool kRolledLoad = T == 6 || T >= 9;
    // Every lane reads and writes its own 32 T contiguous bytes with 16-byte accesses.  Across the lanes of a wave these are
    // strided, but every cache line is used in full within the 2 T accesses of the lane that owns it, and a wide permutation
    // moves 64 T bytes in ~2 ms of arithmetic: nothing to gain from staging the wave's span through LDS, and without the
    // staging code (two barriers, the T-element gather) the register allocation of the permute kernel comes out like that of
    // the hash kernel (no spills inside the rounds).
    // the T elements at g into the registers; `adjust(i, element)` may replace an element on its way in (the absorb driver
    // adds its input there, on the ABI residues, before the bit-slicing - absorb_adjust below)
    template <class Adjust>
    __device__ __forceinline__ void load_elements(const uint4 *g, const Adjust &adjust) {
        if constexpr (kRolledLoad) {
            zero();
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (uint32_t i = 0; i < (uint32_t)T; ++i) set(i, from_abi(adjust(i, abi_from_u4(g[2 * i], g[2 * i + 1]))));
        } else {
            static_for<0, T>([&](auto i) { s[i] = from_abi(adjust((uint32_t)i, abi_from_u4(g[2 * i], g[2 * i + 1]))); });
        }
    }
    struct NoAdjust {
        __device__ __forceinline__ Abi operator()(uint32_t, const Abi &a) const { return a; }
    };
    // state[pos + j] += row[j] for j < count (mod.rs:128,143), as the state comes in: both fully reduced residues, one
    // 256-bit add and one conditional subtraction (abi_add_mod); count is per lane, 0 for a lane that absorbs nothing here
    struct AbsorbAdjust {
        const uint32_t *row, *p32;
        uint32_t pos, count;
        __device__ __forceinline__ Abi operator()(uint32_t i, const Abi &a) const {
            const uint32_t j = i - pos;
            if (j < count) return abi_add_mod(a, abi_load(row + 8 * j), p32);
            return a;
        }
    };
    template <class Adjust = NoAdjust>
    __device__ __forceinline__ void load_states(const uint64_t *g_states, size_t n, const Adjust &adjust = Adjust{}) {
        const size_t gid = (size_t)blockIdx.x * kThreads + threadIdx.x;
        load_elements(reinterpret_cast<const uint4 *>(g_states) + (gid < n ? gid : 0) * kChunks, adjust);
    }

    // the store goes through the wave's LDS region so that every 16-byte write instruction covers 1 KiB of contiguous memory:
    // written lane by lane (stride 32 T bytes) the partial lines are not all merged before they leave the L2 - 1.57 x the
    // bytes at t = 9 (WRITE_SIZE, profiles/r03)
    // (the T exact reductions of a store, once, into the wave's region, between two workgroup barriers)
    __device__ __forceinline__ void stage_abi() {
        __syncthreads();
        static_for<0, T>([&](auto i) {
            const Abi a = to_abi(s[i]);
            region[lane * kChunks + 2 * i] = abi_lo(a);
            region[lane * kChunks + 2 * i + 1] = abi_hi(a);
            PMX_SCHED_FENCE();   // one conversion at a time: interleaved, the T exact reductions are the widest point of the kernel
        });
        __syncthreads();
    }
    // this wave's 64 consecutive states of a batch of n: where their chunks start, and how many of them exist
    struct WaveSpan {
        uint4 *g;
        uint32_t n_chunks;
    };
    __device__ __forceinline__ static WaveSpan wave_span(uint64_t *g_states, size_t n) {
        const size_t first = (size_t)blockIdx.x * kThreads + (threadIdx.x & ~63u);
        const size_t valid = n > first ? (n - first < (size_t)64 ? n - first : (size_t)64) : 0;
        return WaveSpan{reinterpret_cast<uint4 *>(g_states) + first * kChunks, (uint32_t)valid * kChunks};
    }
    __device__ __forceinline__ void store_states(uint64_t *g_states, size_t n) {
        const WaveSpan w = wave_span(g_states, n);
        stage_abi();
#pragma unroll
        for (int k = 0; k < kChunks; ++k) {
            const uint32_t q = lane + k * 64;
            if (q < w.n_chunks) w.g[q] = region[q];
        }
        __syncthreads();
    }

    // One state per lane at a per-lane address (permute_listed_kernel: the sponges of a pass, gathered through an index
    // list).  Every lane reads and writes its own 32 T contiguous bytes with 16-byte accesses: each line is used in full by
    // the lane that owns it.
    __device__ __forceinline__ void load_state_at(const uint64_t *mine, const AbsorbAdjust &add) {
        load_elements(reinterpret_cast<const uint4 *>(mine), add);
    }
    // store_states for the sponges of this wave whose `keep` bit is set (sponge_first_kernel: the permutation ran for the whole
    // workgroup, only the sponges that needed it take its result).  Staged through the wave's region like store_states: a
    // 16-byte write instruction covers whole states, so the predicate travels as the wave's ballot.
    // rate elements copied out of the state that is being stored (squeeze, mod.rs:159-170): out[j] = state[pos + j], j < count,
    // read from the wave's LDS staging, where every element already sits fully reduced in ABI form; count is per lane
    struct CopyOut {
        uint32_t *row;
        uint32_t pos, count;
    };
    __device__ __forceinline__ void copy_out_staged(const CopyOut &out) const {
        for (uint32_t j = 0; j < out.count; ++j) {
            uint4 *dst = reinterpret_cast<uint4 *>(out.row + 8 * j);
            dst[0] = region[lane * kChunks + 2 * (out.pos + j)];
            dst[1] = region[lane * kChunks + 2 * (out.pos + j) + 1];
        }
    }
    __device__ __forceinline__ void store_states_where(uint64_t *g_states, size_t n, uint64_t keep_mask, const CopyOut &out) {
        const WaveSpan w = wave_span(g_states, n);
        stage_abi();
#pragma unroll
        for (int k = 0; k < kChunks; ++k) {
            const uint32_t q = lane + k * 64;
            if (q < w.n_chunks && ((keep_mask >> (q / kChunks)) & 1)) w.g[q] = region[q];
        }
        copy_out_staged(out);
        __syncthreads();
    }

    // `together`: the wave's active lanes hold CONSECUTIVE states starting at wave_base (a prefix of the lanes) - then the
    // wave's span goes out as whole kilobytes like store_states does; otherwise every lane writes its own state.  Either
    // way the T exact reductions happen once, into the wave's LDS region.
    __device__ __forceinline__ void store_state_at(uint64_t *mine, bool keep, bool together, uint64_t *wave_base, uint32_t valid, const CopyOut &out) {
        stage_abi();
        if (together) {          // wave-uniform
            uint4 *g = reinterpret_cast<uint4 *>(wave_base);
            const uint32_t n_chunks = valid * kChunks;
#pragma unroll
            for (int k = 0; k < kChunks; ++k) {
                const uint32_t q = lane + k * 64;
                if (q < n_chunks) g[q] = region[q];
            }
        } else if (keep) {
            uint4 *g = reinterpret_cast<uint4 *>(mine);
#pragma clang loop unroll(disable)
            for (int k = 0; k < kChunks; ++k) g[k] = region[lane * kChunks + k];
        }
        copy_out_staged(out);
        __syncthreads();
    }

    static void describe(EngineInfo &o) {
        std::snprintf(o.engine, sizeof o.engine, "HybridEngine<%d,%d,mfma,windows of %d>", T, ALPHA, mfma_window_for(T));
        o.threads = kThreads;
        o.optimised = 1;
        o.row_tables = mfma_hist_tab(T) ? 1 : 2;   // how the history terms of the S-box inputs are formed: 1 shifted table on the VALU (t = 3), 2 rows on the matrix cores
        o.lane_tables = 0;
        o.mfma_dense = 1;
        o.partial_window = mfma_window_for(T);
    }

    __device__ __forceinline__ Fe get(uint32_t i) const {
        Fe r = s[0];
        static_for<1, T>([&](auto k) {
#pragma unroll
            for (int w = 0; w < kN; ++w) r.l[w] = (i == (uint32_t)k) ? s[k].l[w] : r.l[w];
        });
        return r;
    }
    __device__ __forceinline__ void set(uint32_t i, const Fe &v) {
        static_for<0, T>([&](auto k) {
#pragma unroll
            for (int w = 0; w < kN; ++w) s[k].l[w] = (i == (uint32_t)k) ? v.l[w] : s[k].l[w];
        });
    }

    // lane0_zero: the caller knows lane 0 of the state is zero (pmx_permute.hpp: the window engines skip its round-0 S-box)
    __device__ __forceinline__ void permute(uint32_t want_lo = 0, uint32_t want_hi = T, bool lane0_zero = false) {
        permute_hybrid<T, ALPHA, Scratch, mfma_window_for(T)>(s, sc, tb, c, one, f, want_lo, want_hi, lane0_zero);
    }
};

// The same engine for a modulus that is 1 mod 2^29 (BLS12-381 Fr): its S-boxes take the complemented quotient digits (pmx_field.hpp:
// mont_sqr_p1 / mont_mul_p1), everything else - tables, rows, I/O, the name it reports - is HybridEngine's.  The launcher's choice
// (window_engine below); a kernel of it must never meet another modulus.
template <int T, int ALPHA>
struct HybridEngineP1 : HybridEngine<T, ALPHA> {
    using Base = HybridEngine<T, ALPHA>;
    __device__ __forceinline__ HybridEngineP1(const DevConfig &d, const uint32_t *consts) : Base(d, consts) {}
    __device__ __forceinline__ void permute(uint32_t want_lo = 0, uint32_t want_hi = T, bool lane0_zero = false) {
        permute_hybrid<T, ALPHA, typename Base::Scratch, mfma_window_for(T), true>(this->s, this->sc, this->tb, this->c, this->one, this->f, want_lo, want_hi, lane0_zero);
    }
};

// ------------------------------------------------------------------------------------------------
// LdsEngine: width is a run-time value.  Each wave keeps its 64 states in LDS as
// cur[(element * 9 + limb) * 64 + lane] u32, with a second buffer for the MDS output.
// LDS per wave: 2 buffers x t x 9 x 64 x 4 B  (2.25 t KiB each); the second buffer doubles as the
// staging area of the coalesced ABI load/store (t x 32 B x 64 fits one buffer).
// ------------------------------------------------------------------------------------------------
template <int ALPHA>
struct LdsEngine : LanePerUnit<128> {
    static constexpr int kMinWaves = 1, kMinWavesDriver = 1;
    static constexpr bool kWaveUniformOnly = false;

    Rounds c;
    FieldRt f;
    Fe one;
    const uint32_t *ark;
    const uint32_t *mds;
    uint32_t t;
    uint32_t lane;
    uint32_t *cur;
    uint32_t *nxt;

    static size_t lds_bytes(const DevConfig & /*d*/, uint32_t t) { return (size_t)(kThreads / 64) * 2 * t * kN * 64 * 4; }

    __device__ __forceinline__ LdsEngine(const DevConfig &d, const uint32_t *consts) : c(d.rounds), f(d.field), one(d.one) {
        f.io = consts + d.io_offset;
        ark = consts;
        mds = consts + d.mds_offset;
        t = c.rate + c.capacity;
        lane = threadIdx.x & 63;
        const uint32_t wave = threadIdx.x >> 6;
        cur = reinterpret_cast<uint32_t *>(pmx_lds) + (size_t)wave * 2 * (t * kN * 64);
        nxt = cur + t * kN * 64;
    }

    __device__ __forceinline__ Fe get(uint32_t i) const {
        Fe r;
#pragma unroll
        for (int w = 0; w < kN; ++w) r.l[w] = cur[(i * kN + w) * 64 + lane];
        return r;
    }
    __device__ __forceinline__ void set(uint32_t i, const Fe &v) {
#pragma unroll
        for (int w = 0; w < kN; ++w) cur[(i * kN + w) * 64 + lane] = v.l[w];
    }
    __device__ __forceinline__ void set_next(uint32_t i, const Fe &v) {
#pragma unroll
        for (int w = 0; w < kN; ++w) nxt[(i * kN + w) * 64 + lane] = v.l[w];
    }
    __device__ __forceinline__ void swap() {
        uint32_t *tmp = cur;
        cur = nxt;
        nxt = tmp;
    }

    __device__ __forceinline__ void zero() {
        for (uint32_t i = 0; i < t; ++i) set(i, fe_zero());
    }
    __device__ __forceinline__ Fe from_abi(const Abi &x) const { return fe_from_abi(x, f); }            // dense schedule: exact conversions
    __device__ __forceinline__ Abi to_abi(const Fe &x) const { return fe_to_abi(x, f); }

    // wave-level: 64 contiguous ABI states = 64*2t contiguous 16-B chunks in global memory, staged through
    // the `nxt` buffer (chunk q of the wave at uint4 index q), then converted element by element
    __device__ __forceinline__ void load_states(const uint64_t *g_states, size_t n) {
        const size_t first = ((size_t)blockIdx.x * kThreads + (threadIdx.x & ~63u));
        const size_t valid = n > first ? (n - first < 64 ? n - first : 64) : 0;
        const uint32_t chunks = 2 * t;
        const uint4 *g = reinterpret_cast<const uint4 *>(g_states) + first * chunks;
        const uint32_t n_chunks = (uint32_t)valid * chunks;
        uint4 *st = reinterpret_cast<uint4 *>(nxt);
        __syncthreads();
        for (uint32_t k = 0; k < chunks; ++k) {
            const uint32_t q = lane + k * 64;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (q < n_chunks) v = g[q];
            st[q] = v;
        }
        __syncthreads();
        for (uint32_t i = 0; i < t; ++i) set(i, from_abi(abi_from_u4(st[lane * chunks + 2 * i], st[lane * chunks + 2 * i + 1])));
        __syncthreads();
    }

    __device__ __forceinline__ void store_states(uint64_t *g_states, size_t n) {
        const size_t first = ((size_t)blockIdx.x * kThreads + (threadIdx.x & ~63u));
        const size_t valid = n > first ? (n - first < 64 ? n - first : 64) : 0;
        const uint32_t chunks = 2 * t;
        uint4 *g = reinterpret_cast<uint4 *>(g_states) + first * chunks;
        const uint32_t n_chunks = (uint32_t)valid * chunks;
        uint4 *st = reinterpret_cast<uint4 *>(nxt);
        __syncthreads();
        for (uint32_t i = 0; i < t; ++i) {
            const Abi a = to_abi(get(i));
            st[lane * chunks + 2 * i] = abi_lo(a);
            st[lane * chunks + 2 * i + 1] = abi_hi(a);
        }
        __syncthreads();
        for (uint32_t k = 0; k < chunks; ++k) {
            const uint32_t q = lane + k * 64;
            if (q < n_chunks) g[q] = st[q];
        }
        __syncthreads();
    }

    static void describe(EngineInfo &o) {
        std::snprintf(o.engine, sizeof o.engine, "LdsEngine<%d>", ALPHA);
        o.threads = kThreads;
        o.optimised = o.row_tables = o.lane_tables = o.mfma_dense = 0;
    }

    __device__ __forceinline__ void permute(uint32_t /*want_lo*/ = 0, uint32_t /*want_hi*/ = PMX_MAX_WIDTH, bool /*lane0_zero*/ = false) {
        uint32_t *const home = cur;
        permute_dense_rt<ALPHA>(*this, t, ark, mds, c, one, f);
        // Lanes may permute a different number of times (per-sponge modes) while load/store_states use the
        // wave-uniform `nxt` as staging: always leave the state in the buffer it started in.
        if (cur != home) {
            for (uint32_t q = 0; q < t * kN; ++q) nxt[q * 64 + lane] = cur[q * 64 + lane];
            swap();
        }
    }
};

// ------------------------------------------------------------------------------------------------
// QuadEngine: ONE state spread over a quad of lanes (pmx_permute.hpp, cooperative schedule; t = 3): lane q of a quad
// holds state element q, lane 3 is the spare that squares in the folded sparse rounds; the values a round exchanges
// travel by quad-broadcast DPP moves.  For latency-bound launches - the narrow levels of a tree, a handful of sponges -
// where what is paid is the length of one permutation's dependent chain: 32 k instructions here, 58-67 k with one lane
// per state.  LDS: the cooperative table, staged once per workgroup (256 threads = 64 states).
// Unit g is quad threadIdx.x / 4 of its workgroup; lanes 0..2 move their element in and out, lane 0 writes the mode words.
// Every per-unit value of a kernel (active, the mode words, the cursors of the driver) is the same in the four lanes of a
// quad, so whole quads are active or inactive together - which permute() needs: its DPP moves read the other lanes of the quad.
// ------------------------------------------------------------------------------------------------
template <int ALPHA>
struct QuadEngine {
    static constexpr int kThreads = 256, kUnits = 64;
    static constexpr int kMinWaves = 2, kMinWavesDriver = 2;
    static constexpr bool kWaveUniformOnly = false;   // quads diverge as units

    Rounds c;
    FieldRt f;
    Fe one;
    const uint32_t *coop;
    uint32_t q, role;
    Fe s;   // this lane's element of its quad's state

    static size_t lds_bytes(const DevConfig &d, uint32_t /*t*/) { return (size_t)d.rounds.total_rounds * 3 * kCoopElems * kFeStride * 4; }

    // the table is staged by the whole workgroup behind a barrier: every kernel builds its engine before any lane can leave
    __device__ __forceinline__ QuadEngine(const DevConfig &d, const uint32_t *consts) : c(d.rounds), f(d.field), one(d.one) {
        f.io = consts + d.io_offset;
        const uint32_t table_chunks = c.total_rounds * 3 * kCoopElems * kFeStride / 4;
        const uint4 *g4 = reinterpret_cast<const uint4 *>(consts + d.coop_offset);
        for (uint32_t k = threadIdx.x; k < table_chunks; k += kThreads) pmx_lds[k] = g4[k];
        __syncthreads();
        coop = reinterpret_cast<const uint32_t *>(pmx_lds);
        q = threadIdx.x & 3;
        role = q < 3 ? q : 2;   // lane 3 reads lane 2's entries; in the uniform rounds it shadows lane 2 (its result is never read)
        s = fe_zero();
    }

    __device__ __forceinline__ static size_t unit() { return (size_t)blockIdx.x * kUnits + (threadIdx.x >> 2); }
    __device__ __forceinline__ bool owns(uint32_t i) const { return q == i; }
    __device__ __forceinline__ bool writes_mode() const { return q == 0; }   // once per sponge

    // get / set / zero act on the lane's own element: the kernels ask owns(i) before they store or add into element i
    __device__ __forceinline__ Fe get(uint32_t /*i*/) const { return s; }
    __device__ __forceinline__ void set(uint32_t /*i*/, const Fe &v) { s = v; }
    __device__ __forceinline__ void zero() { s = fe_zero(); }
    __device__ __forceinline__ Fe from_abi(const Abi &x) const { return fe_from_abi_scaled(x); }      // the optimised schedule carries the ABI residue as its internal form (pmx_field.hpp: fe_from_abi_scaled)
    __device__ __forceinline__ Abi to_abi(const Fe &x) const { return fe_to_abi_scaled(x, f); }

    // lanes 0..2 of the quad of unit g read / write element q of state g (any rate / capacity split of width 3)
    uint32_t *mine;   // (the address is formed once, by load_states, and kept for store_states)
    __device__ __forceinline__ void load_states(uint64_t *g_states, size_t n) {
        const size_t g = unit();
        mine = reinterpret_cast<uint32_t *>(g_states + ((g < n ? g : 0) * 3 + role) * 4);
        if (g < n && q < 3) s = from_abi(abi_load(mine));
    }
    __device__ __forceinline__ void store_states(uint64_t * /*g_states*/, size_t n) {
        const Abi v = to_abi(s);
        if (unit() < n && q < 3) abi_store(mine, v);
    }

    static void describe(EngineInfo &o) {
        std::snprintf(o.engine, sizeof o.engine, "QuadEngine<%d>", ALPHA);
        o.threads = kThreads;   // 64 states, one per quad of lanes
        o.optimised = 1;        // element form, sparse rounds folded three multiplications deep
        o.row_tables = o.lane_tables = o.mfma_dense = 0;
    }

    // element held by lane `lane` of this quad, in every lane
    template <int LANE>
    __device__ __forceinline__ static Fe quad(const Fe &v) {
        Fe r;
#pragma unroll
        // quad_perm [l, l, l, l]; every lane reads a live lane of its own quad, so there is no "old" value to keep: mov_dpp,
        // not update_dpp(0, ...), which costs a v_mov_b32 of the 0 before every move (27 per round on a lone wave's chain)
        for (int w = 0; w < kN; ++w) r.l[w] = (uint32_t)__builtin_amdgcn_mov_dpp((int)v.l[w], LANE * 0x55, 0xf, 0xf, false);
        return r;
    }

    // the whole state every time (the arguments are the window engines' hints); called by whole quads (see above)
    __device__ __forceinline__ void permute(uint32_t /*want_lo*/ = 0, uint32_t /*want_hi*/ = 3, bool /*lane0_zero*/ = false) {
        const uint32_t first_partial = c.half_full, last_partial = c.half_full + c.partial_rounds - 1;
        for (uint32_t r = 0; r < c.total_rounds; ++r) {
            const uint32_t *entry = coop + ((size_t)r * 3 + role) * kCoopElems * kFeStride;
            if (kCoopFolded<ALPHA> && r >= first_partial && r < last_partial) {   // sparse round, three multiplications deep
                const Fe x = quad<0>(fe_add_lazy(s, fe_const(entry)));
                const Fe res_a = coop_fold_a(q, x, entry, f);
                const Fe res_b = coop_fold_b(q, s, res_a, entry, f);
                Fe xpow = res_b;
#pragma unroll
                for (int k = 0; k < kCoopExtraSquarings<ALPHA>; ++k) xpow = mont_sqr(xpow, f);
                s = coop_fold_c(q, s, quad<3>(xpow), res_a, quad<1>(res_b), quad<2>(res_b), f);
                continue;
            }
            const Fe z = coop_pre<ALPHA>(s, entry, is_full_round(r, c) || q == 0, c, one, f);
            Fe zz[3];
            zz[0] = quad<0>(z);
            zz[1] = quad<1>(z);
            zz[2] = quad<2>(z);
            s = coop_layer_is_norm(r, c) ? coop_post_norm(zz, entry, f) : coop_post(zz, entry, f);
        }
        // lane 3 carries scratch values through the rounds; keep them bounded for the next call's lazy adds
        if (q == 3) s = fe_zero();
    }
};

}  // namespace pmx
