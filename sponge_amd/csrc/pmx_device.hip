// gfx950 kernels of the batched Poseidon permutation and duplex-sponge driver, plus their launchers.
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
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "../../include/poseidon_mi355x.h"
#include "pmx_field.hpp"
#include "pmx_internal.hpp"
#include "pmx_launch.hpp"
#include "pmx_permute.hpp"
#include "pmx_sponge_plan.hpp"

// The file is compiled nine times (Makefile, in parallel): PMX_TU = 0 holds the quad engine, the run-time-width engine and the
// public launchers; PMX_TU = 1 / 3 hold the hybrid engines for alpha = 5 (widths up to 6 / from 7), PMX_TU = 2 / 4 the same for the
// generic S-box (each width x 7 kernels - by far the longest compile), PMX_TU = 5 .. 8 those four for a modulus that is 1 mod 2^29.
#ifndef PMX_TU
#define PMX_TU 0
#endif

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

// ------------------------------------------------------------------------------------------------
// Kernels (shared by the three engines).  The engine says where a unit lives: unit() and kUnits per workgroup, owns(i) - this
// lane holds element i, so it stores it and adds an absorbed element into it - and writes_mode() - this lane writes the
// sponge's mode words, once per sponge.  With one lane per unit (LanePerUnit) they fold to the lane index and `true`.
// Every kernel builds its engine before any lane can leave (QuadEngine stages its table into LDS behind a barrier).
// ------------------------------------------------------------------------------------------------
template <class Engine>
__global__ void __launch_bounds__(Engine::kThreads, Engine::kMinWaves) permute_kernel(const DevConfig d, const uint32_t *__restrict__ consts, uint64_t *__restrict__ states, size_t n) {
    Engine e(d, consts);
    e.load_states(states, n);
    // (all lanes of the result are wanted; the width is passed as the run-time value it also is in the other kernels: with the
    // compile-time constant the wide engines' last round is specialised and the register allocation of the whole kernel
    // comes out worse - 132 instead of 0..20 bytes of scratch per lane at t = 9, spills inside the sparse rounds)
    e.permute(0, e.c.rate + e.c.capacity);
    e.store_states(states, n);
}

// Where the input rows of an absorb call live (absorb_kernel, sponge_walk, sponge_first_kernel, permute_listed_kernel): a policy
// that hands out one sponge's Row - its length, the address of its element `first`, whether any pass walks it and where its walk ends.
//   RowsFixed    every row `len` elements, row i at io + i * len (pmx_sponge_absorb_batch*, and the squeeze side of every call)
//   RowsRagged   row i is [offsets[i], offsets[i + 1]) clamped to max_len (pmx_sponge_absorb_varlen_batch*, pmx_sponge_plan.hpp):
//                the two offsets are loaded once per sponge in front of a kernel's permutation (and again behind it: refetch); an empty
//                row is walked by no pass, and a sponge's walk ends at ITS last pass, the one that moves the end of its row, not the call's
struct RowsFixed {
    size_t len;
    struct Row {
        size_t sponge, len;
        __device__ __forceinline__ size_t length() const { return len; }
        template <class P>
        __device__ __forceinline__ P *at(P *io, uint32_t first) const { return io + (sponge * len + first) * 4; }
        __device__ __forceinline__ static constexpr bool walks() { return true; }
        __device__ __forceinline__ bool ends(uint32_t q, uint32_t call_last, const SpongePass &) const { return q >= call_last; }
    };
    __device__ __forceinline__ Row row(size_t sponge, bool /*active*/) const { return Row{sponge, len}; }
    __device__ __forceinline__ Row refetch(size_t sponge, bool active) const { return row(sponge, active); }
    size_t bound() const { return len; }
};
struct RowsRagged {
    const uint64_t *in;        // the input: row i starts at in + offsets[i] (the kernels' own `io` argument is not read)
    const uint64_t *offsets;   // [n + 1], device-resident, not validated (see varlen_row_len)
    uint32_t max_len;          // the caller's bound on every row; sets the call's passes
    struct Row {
        const uint64_t *base;  // the row's first element
        uint32_t len;
        __device__ __forceinline__ size_t length() const { return len; }
        template <class P>
        __device__ __forceinline__ P *at(P * /*io*/, uint32_t first) const { return const_cast<P *>(base) + (size_t)first * 4; }
        __device__ __forceinline__ bool walks() const { return absorb_row_walks(len); }
        // (the call's last pass as a backstop: it is never reached first - pmx_sponge_plan.hpp, tests/test_varlen_plan.py)
        __device__ __forceinline__ bool ends(uint32_t q, uint32_t call_last, const SpongePass &sp) const { return absorb_row_ends(sp, len) || q >= call_last; }
    };
    // (an inactive lane reads nothing: its Row is empty)
    __device__ __forceinline__ Row row(size_t sponge, bool active) const {
        if (!active) return Row{in, 0};
        const uint64_t lo = offsets[sponge], hi = offsets[sponge + 1];
        return Row{in + lo * 4, varlen_row_len(lo, hi, max_len)};
    }
    // the same Row behind the permutation of a pass kernel, loaded again: kept in registers across the permutation it spilled (t = 9: 12
    // bytes of scratch in the listed kernel).
    // The empty asm makes the pointer opaque, so that the compiler issues the two loads again instead of keeping the first ones.
    __device__ __forceinline__ Row refetch(size_t sponge, bool active) const {
        RowsRagged again = *this;
        asm volatile("" : "+s"(again.offsets));
        return again.row(sponge, active);
    }
    size_t bound() const { return max_len; }
};

// absorb `in_len` elements into this lane's sponge; idx is the next absorb index, or `rate` to force the
// permutation a Squeezing sponge performs first (mod.rs:247-252).  Returns the final next_absorb_index.
// The reference walks the input element by element and permutes whenever the rate is full and more input remains
// (mod.rs:137-148).  Sponges of one wave may stand at different positions, and a permutation costs the wave the same
// whether one lane needs it or all 64: so every lane keeps its OWN input cursor, and a pass of the loop is "every lane
// absorbs until its rate is full or its input ends, then the lanes that are full and have input left permute together".
// A wave then executes max-over-lanes permutations (2 for absorb(4) at rate 2 whatever the positions) instead of one per
// input position at which some lane happens to be full (4).
template <class Engine>
__device__ __forceinline__ uint32_t absorb_elements(Engine &e, const uint64_t *row, size_t in_len, uint32_t idx,
                                                    bool active) {
    const Rounds &c = e.c;
    size_t k = active ? 0 : in_len;   // this lane's cursor into its input row
    while (__builtin_amdgcn_ballot_w64(k < in_len)) {
        for (uint32_t j = 0; j < c.rate; ++j) {   // wave-uniform trip count; lanes drop out as they fill up or run dry
            if (k < in_len && idx < c.rate) {
                const Fe x = e.from_abi(abi_load(reinterpret_cast<const uint32_t *>(row + 4 * k)));
                const uint32_t pos = c.capacity + idx;
                // state[capacity + idx] += element (mod.rs:128,143); normalised so the permutation's own lazy
                // round-constant add stays within the limb bounds
                if (e.owns(pos)) e.set(pos, fe_normalize(fe_add_lazy(e.get(pos), x)));
                idx += 1;
                k += 1;
            }
        }
        // rate filled and more input remains -> permute (mod.rs:137-148; also the :241-252 cases)
        const bool need = k < in_len && idx == c.rate;
        if (__builtin_amdgcn_ballot_w64(need)) {
            if (need) {
                e.permute();
                idx = 0;
            }
        }
    }
    return idx;
}

// squeeze_internal (mod.rs:153-182) preceded by the mode handling of mod.rs:323-338.
// `need` = permute before the first copy.  Returns the final next_squeeze_index.
template <class Engine>
__device__ __forceinline__ uint32_t squeeze_elements(Engine &e, uint64_t *row, size_t out_len, uint32_t idx, bool need,
                                                     bool active) {
    const Rounds &c = e.c;
    size_t rem = out_len;
    size_t pos = 0;
    bool done = !active;
    while (__builtin_amdgcn_ballot_w64(!done)) {
        const bool do_perm = !done && need;
        if (__builtin_amdgcn_ballot_w64(do_perm)) {
            if (do_perm) e.permute();
        }
        if (!done) {
            const bool last = idx + rem <= c.rate;
            const uint32_t take = last ? (uint32_t)rem : c.rate - idx;
            for (uint32_t k = 0; k < take; ++k) {
                const uint32_t i = c.capacity + idx + k;
                if (e.owns(i)) abi_store(reinterpret_cast<uint32_t *>(row + 4 * (pos + k)), e.to_abi(e.get(i)));
            }
            if (last) {
                idx += take;
                done = true;
            } else {
                need = rem != c.rate;  // mod.rs:175, tested before the slice is advanced
                rem -= take;
                pos += take;
                idx = 0;
            }
        }
    }
    return idx;
}

// Fixed-shape hash: every row runs  new; absorb(in_len elements); squeeze_native(out_len)  with the same lengths,
// so the whole state machine is wave-uniform.  It is written as ONE loop around ONE permutation call site (the
// permutation is the bulk of the kernel's code; two inlined copies overflow the instruction cache at t = 9).
template <class Engine>
__global__ void __launch_bounds__(Engine::kThreads, Engine::kMinWaves)
    hash_kernel(const DevConfig d, const uint32_t *__restrict__ consts, const uint64_t *__restrict__ in, size_t in_len,
                uint64_t *__restrict__ out, size_t out_len, size_t n) {
    Engine e(d, consts);
    const Rounds &c = e.c;
    const size_t gid = Engine::unit();
    const bool active = gid < n;
    e.zero();                                                  // CryptographicSponge::new, mod.rs:219-230
    const uint64_t *row_in = in + (active ? gid : 0) * in_len * 4;
    uint64_t *row_out = out + (active ? gid : 0) * out_len * 4;
    size_t k_in = 0, rem = out_len, pos = 0;
    uint32_t idx = 0;
    bool squeezing = false, need = false;
    bool fresh = c.capacity >= 1;   // until the first permutation the capacity lanes of the new sponge - lane 0 among them - are zero
    // The sponge is dropped when the row is done, so the LAST permutation only has to produce the lanes the last squeeze
    // copies out: [capacity, capacity + rem) once rem <= rate elements are left (want_hi; otherwise the whole state).
    const uint32_t t_all = c.rate + c.capacity;
    uint32_t want_hi = t_all;
    for (;;) {
        if (need) {
            e.permute(want_hi < t_all ? c.capacity : 0, want_hi, fresh);
            need = false;
            fresh = false;
        }
        if (k_in < in_len) {                                   // absorb_internal, mod.rs:121-150
            if (idx == c.rate) {                               // rate full and more input remains
                need = true;
                idx = 0;
                continue;
            }
            Fe x = fe_zero();
            if (active) x = e.from_abi(abi_load(reinterpret_cast<const uint32_t *>(row_in + 4 * k_in)));
            const uint32_t at = c.capacity + idx;
            if (e.owns(at)) e.set(at, fe_normalize(fe_add_lazy(e.get(at), x)));
            ++idx;
            ++k_in;
            continue;
        }
        if (!squeezing) {                                      // Absorbing -> permute, squeeze from 0 (mod.rs:324-328)
            squeezing = true;
            need = true;
            idx = 0;
            if (rem <= c.rate) want_hi = c.capacity + (uint32_t)rem;
            continue;
        }
        const bool last = idx + rem <= c.rate;                 // squeeze_internal, mod.rs:153-182
        const uint32_t take = last ? (uint32_t)rem : c.rate - idx;
        for (uint32_t k = 0; k < take; ++k) {
            const uint32_t i = c.capacity + idx + k;
            const Abi v = e.to_abi(e.get(i));
            if (active && e.owns(i)) abi_store(reinterpret_cast<uint32_t *>(row_out + 4 * (pos + k)), v);
        }
        if (last) break;
        need = rem != c.rate;                                  // mod.rs:175, tested before the slice is advanced
        rem -= take;
        pos += take;
        idx = 0;
        if (need && rem <= c.rate) want_hi = c.capacity + (uint32_t)rem;
    }
}

// The same rows out of a matrix (pmx_matrix_*; pmx_matrix_shape.hpp has the strides of a layout): element k of row gid is at
// in + (gid * row_stride + k * elem_stride) * 4.  Row-major rows are (row_len, 1), hash_kernel's own addressing; a column-major matrix
// of leading dimension ld is (1, ld), where the units of a wave read consecutive elements - 2 KB in one piece per absorbed element.
// hash_kernel's state machine word for word: ONE loop around ONE permutation call site, want_hi, fresh, an inactive lane loads nothing,
// and every lane of a unit loads the element while the lane that owns its state element keeps it.  The input cursor is a pointer that
// advances by the element stride, so the absorb path holds no multiplication.  A twin and not a parameter of hash_kernel: the kernel
// behind pmx_hash_batch[_dev] stays the code it was.
template <class Engine>
__global__ void __launch_bounds__(Engine::kThreads, Engine::kMinWaves)
    hash_strided_kernel(const DevConfig d, const uint32_t *__restrict__ consts, const uint64_t *__restrict__ in, size_t in_len, size_t row_stride,
                        size_t elem_stride, uint64_t *__restrict__ out, size_t out_len, size_t n) {
    Engine e(d, consts);
    const Rounds &c = e.c;
    const size_t gid = Engine::unit();
    const bool active = gid < n;
    e.zero();                                                  // CryptographicSponge::new, mod.rs:219-230
    const uint64_t *next_in = in + (active ? gid : 0) * row_stride * 4;   // element k_in of this unit's row
    uint64_t *row_out = out + (active ? gid : 0) * out_len * 4;
    size_t k_in = 0, rem = out_len, pos = 0;
    uint32_t idx = 0;
    bool squeezing = false, need = false;
    bool fresh = c.capacity >= 1;   // (see hash_kernel)
    const uint32_t t_all = c.rate + c.capacity;
    uint32_t want_hi = t_all;
    for (;;) {
        if (need) {
            e.permute(want_hi < t_all ? c.capacity : 0, want_hi, fresh);
            need = false;
            fresh = false;
        }
        if (k_in < in_len) {                                   // absorb_internal, mod.rs:121-150
            if (idx == c.rate) {                               // rate full and more input remains
                need = true;
                idx = 0;
                continue;
            }
            Fe x = fe_zero();
            if (active) x = e.from_abi(abi_load(reinterpret_cast<const uint32_t *>(next_in)));
            const uint32_t at = c.capacity + idx;
            if (e.owns(at)) e.set(at, fe_normalize(fe_add_lazy(e.get(at), x)));
            ++idx;
            ++k_in;
            next_in += elem_stride * 4;
            continue;
        }
        if (!squeezing) {                                      // Absorbing -> permute, squeeze from 0 (mod.rs:324-328)
            squeezing = true;
            need = true;
            idx = 0;
            if (rem <= c.rate) want_hi = c.capacity + (uint32_t)rem;
            continue;
        }
        const bool last = idx + rem <= c.rate;                 // squeeze_internal, mod.rs:153-182
        const uint32_t take = last ? (uint32_t)rem : c.rate - idx;
        for (uint32_t k = 0; k < take; ++k) {
            const uint32_t i = c.capacity + idx + k;
            const Abi v = e.to_abi(e.get(i));
            if (active && e.owns(i)) abi_store(reinterpret_cast<uint32_t *>(row_out + 4 * (pos + k)), v);
        }
        if (last) break;
        need = rem != c.rate;                                  // mod.rs:175, tested before the slice is advanced
        rem -= take;
        pos += take;
        idx = 0;
        if (need && rem <= c.rate) want_hi = c.capacity + (uint32_t)rem;
    }
}

// 2-to-1 compression, the Merkle-tree primitive:  out = (new; absorb([l, r]); squeeze_native(1))[0]
//   = permute(state with state[capacity] = l, state[capacity+1] = r, rest 0)[capacity]      (rate >= 2),
// because absorbing rate-many-or-fewer elements into a fresh sponge permutes exactly once, at the squeeze
// (src/poseidon/mod.rs:126-135, 324-328).  One permutation site, 64 contiguous bytes in and 32 out per lane.
template <class Engine>
__global__ void __launch_bounds__(Engine::kThreads, Engine::kMinWaves)
    compress_kernel(const DevConfig d, const uint32_t *__restrict__ consts, const uint64_t *__restrict__ in,
                    uint64_t *__restrict__ out, size_t n) {
    Engine e(d, consts);
    const size_t gid = Engine::unit();
    const bool active = gid < n;
    const uint32_t *pair = reinterpret_cast<const uint32_t *>(in + (active ? gid : 0) * 8);
    e.zero();
    // each input element is loaded by the lane that holds it only
    if (e.owns(e.c.capacity)) e.set(e.c.capacity, e.from_abi(abi_load(pair)));
    if (e.owns(e.c.capacity + 1)) e.set(e.c.capacity + 1, e.from_abi(abi_load(pair + 8)));
    e.permute(e.c.capacity, e.c.capacity + 1, e.c.capacity >= 1);   // only the digest lane of the result is read; lane 0 (capacity) went in as zero
    const Abi digest = e.to_abi(e.get(e.c.capacity));
    if (active && e.owns(e.c.capacity)) abi_store(reinterpret_cast<uint32_t *>(out + gid * 4), digest);
}

// arity-to-1 compression, the primitive of the wide trees (2 <= arity <= rate, a run-time value):
//   out = (new; absorb([c_0 .. c_{arity-1}]); squeeze_native(1))[0]
//       = permute(state with state[capacity + j] = c_j for j < arity, rest 0)[capacity]
// for the same reason as above (mod.rs:126-135, 219-230, 324-328).  One permutation site, 32 arity contiguous bytes in and 32 out
// per unit; the rate lanes from `arity` on stay the zeros of e.zero().  The child loop stays rolled: its body selects the state
// element at run time, and unrolled rate times it is more code than it is worth in front of the permutation.
template <class Engine>
__global__ void __launch_bounds__(Engine::kThreads, Engine::kMinWaves)
    compress_ary_kernel(const DevConfig d, const uint32_t *__restrict__ consts, const uint64_t *__restrict__ in, uint32_t arity,
                        uint64_t *__restrict__ out, size_t n) {
    Engine e(d, consts);
    const size_t gid = Engine::unit();
    const bool active = gid < n;
    const uint32_t *row = reinterpret_cast<const uint32_t *>(in + (active ? gid : 0) * (size_t)arity * 4);
    e.zero();
#pragma clang loop unroll(disable)
    for (uint32_t j = 0; j < arity; ++j) {
        const uint32_t at = e.c.capacity + j;
        // each child is loaded by the lane that holds its state element only
        if (e.owns(at)) e.set(at, e.from_abi(abi_load(row + 8 * j)));
    }
    e.permute(e.c.capacity, e.c.capacity + 1, e.c.capacity >= 1);   // only the digest lane of the result is read; lane 0 (capacity) went in as zero
    const Abi digest = e.to_abi(e.get(e.c.capacity));
    if (active && e.owns(e.c.capacity)) abi_store(reinterpret_cast<uint32_t *>(out + gid * 4), digest);
}

// The same for a level whose last row is short (pmx_merkle_ragged*: a level of n_children nodes that is no multiple of the arity, or of
// the rate at arity 2): a bounded twin of compress_ary_kernel, as RowsRagged is of RowsFixed - parent gid absorbs the children
// gid * arity .. min((gid + 1) * arity, n_children) - 1 and loads nothing at or beyond n_children (the rows behind the level are the next
// level's nodes, which this very launch writes).  The rate lanes of the children that do not exist keep the zeros of e.zero(): the state of
// (new; absorb(the r children that exist)), mod.rs:126-135 - still one permutation.  The bound is a predicate on the rolled child loop, so
// the loop's trip count stays wave-uniform; it serves every arity, 2 included (the quad engine: a quad shares its unit, so its `have`).
// A level that divides by the arity never comes here (launch_compress_level): the full-row kernels above are what they were.
template <class Engine>
__global__ void __launch_bounds__(Engine::kThreads, Engine::kMinWaves)
    compress_ary_bounded_kernel(const DevConfig d, const uint32_t *__restrict__ consts, const uint64_t *__restrict__ in, uint32_t arity,
                                size_t n_children, uint64_t *__restrict__ out, size_t n) {
    Engine e(d, consts);
    const size_t gid = Engine::unit();
    const bool active = gid < n;
    const size_t first = (active ? gid : 0) * (size_t)arity;
    // children this parent has: arity, fewer for the last parent, none for a lane that is no parent
    const uint32_t have = active && first < n_children ? (n_children - first < (size_t)arity ? (uint32_t)(n_children - first) : arity) : 0;
    const uint32_t *row = reinterpret_cast<const uint32_t *>(in + first * 4);
    e.zero();
#pragma clang loop unroll(disable)
    for (uint32_t j = 0; j < arity; ++j) {
        const uint32_t at = e.c.capacity + j;
        if (j < have && e.owns(at)) e.set(at, e.from_abi(abi_load(row + 8 * j)));
    }
    e.permute(e.c.capacity, e.c.capacity + 1, e.c.capacity >= 1);   // only the digest lane of the result is read; lane 0 (capacity) went in as zero
    const Abi digest = e.to_abi(e.get(e.c.capacity));
    if (active && e.owns(e.c.capacity)) abi_store(reinterpret_cast<uint32_t *>(out + gid * 4), digest);
}

// Proof-of-work grinding on ONE sponge (pmx_sponge_grind; include/poseidon_mi355x.h has the contract): unit gid tries the nonce
// v = first + gid, i.e. the state  base; state[capacity + index] += F::from(v); permute  (mod.rs:232-254 at Absorbing{index}, index <
// rate - the launcher has already performed the permutation the other modes start with), and accepts v when the low `bits` bits of the
// canonical integer of state[capacity] - the first element a squeeze would hand out, mod.rs:272-286 - are zero.  best[0] starts at
// UINT64_MAX and ends as the smallest accepted nonce of the launch; best[1] starts at 0 and ends as 1 if there is one.
// No per-candidate memory: `base` is one row of t ABI elements at a wave-uniform address (scalar loads, 32 t bytes for everybody),
// each loaded by the lane that holds it; the nonce's residue costs one Montgomery product (abi_from_u64) in front of the permutation
// on the quad and window engines, whose from_abi is a bit-slice - two on the run-time-width engine, whose from_abi is an exact
// conversion of its own (against the t^2 products per round of its dense schedule) -,
// and only the digest lane of the last layer is computed, as in compress_kernel.  One atomic per wave at most, in the shape of
// sponge_queue: lanes are in nonce order, so the lowest accepting lane of the ballot holds the wave's smallest nonce.
// A workgroup whose first nonce lies above a nonce already found leaves before it permutes - nothing it could find would lower the
// minimum, so the result stays exact whatever the launch geometry and the order the workgroups run in.  `best` is written by other
// workgroups of this very launch: it is read with a device-scope atomic load, past the scalar cache and the vector L1, like the
// lists of permute_listed_kernel.  (The exit is taken behind the engine's construction - QuadEngine stages its table behind a
// barrier - and no engine's permutation holds a workgroup barrier.)
template <class Engine>
__global__ void __launch_bounds__(Engine::kThreads, Engine::kMinWaves)
    grind_kernel(const DevConfig d, const uint32_t *__restrict__ consts, const uint64_t *__restrict__ base, uint32_t index, uint32_t bits,
                 uint64_t first, size_t n, uint64_t *__restrict__ best) {
    Engine e(d, consts);
    // (one value per wave - the first lane's - so the exit is wave-uniform by construction and a scalar branch: no lane reaches the
    // lane-pair exchange of permute_hybrid or the quad moves with its partner gone.  Waves of one workgroup may see different values
    // and decide differently; the answer is exact either way, because any value seen is a nonce some wave has accepted.)
    const uint64_t seen = __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t found = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)seen) |
                           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(seen >> 32)) << 32);
    if (found < first + (uint64_t)blockIdx.x * Engine::kUnits) return;   // (blockIdx.x * kUnits < n: the sum does not wrap)
    const size_t gid = Engine::unit();
    const bool active = gid < n;
    const uint64_t nonce = first + gid;
    const uint32_t t_all = e.c.rate + e.c.capacity, at = e.c.capacity + index;
    const uint32_t *row = reinterpret_cast<const uint32_t *>(base);
    e.zero();
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < t_all; ++i) {
        if (e.owns(i)) e.set(i, e.from_abi(abi_load(row + 8 * i)));
    }
    // state[capacity + index] += F::from(nonce) (mod.rs:128), normalised like every absorbed element (absorb_elements)
    const Fe x = e.from_abi(abi_from_u64(nonce, e.f));
    if (e.owns(at)) e.set(at, fe_normalize(fe_add_lazy(e.get(at), x)));
    e.permute(e.c.capacity, e.c.capacity + 1);   // only the digest lane of the result is read
    const Abi digest = abi_to_canonical(e.to_abi(e.get(e.c.capacity)), e.f);
    const bool hit = active && e.owns(e.c.capacity) && canonical_low_bits_zero(digest, bits);
    const uint64_t hits = __builtin_amdgcn_ballot_w64(hit);
    if (hits && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(hits)) {
        atomicMin(reinterpret_cast<unsigned long long *>(best), (unsigned long long)nonce);
        best[1] = 1;   // (every writer writes the same value; the nonce 2^64 - 1 is a nonce like any other, not "none")
    }
}

// (per-lane engines: every lane keeps its own cursor and length - lanes of a wave may absorb rows of different lengths; a lane whose
// row is empty absorbs nothing and leaves its mode words alone, mod.rs:234-236)
template <class Engine, class Rows>
__global__ void __launch_bounds__(Engine::kThreads, Engine::kMinWavesDriver)
    absorb_kernel(const DevConfig d, const uint32_t *__restrict__ consts, uint64_t *__restrict__ states,
                  uint32_t *__restrict__ mode_tag, uint32_t *__restrict__ mode_index, const uint64_t *__restrict__ in,
                  Rows rows, size_t n) {
    static_assert(!Engine::kWaveUniformOnly, "this engine's permutation cannot run under the per-lane EXEC masks of absorb_elements");
    Engine e(d, consts);
    const size_t gid = Engine::unit();
    const bool active = gid < n;
    e.load_states(states, n);
    const typename Rows::Row row = rows.row(active ? gid : 0, active);
    uint32_t idx = 0;
    if (active) idx = (mode_tag[gid] == PMX_MODE_ABSORBING) ? mode_index[gid] : e.c.rate;
    if (idx > e.c.rate) idx = e.c.rate;                        // device-resident mode words are not validated by the host
    idx = absorb_elements(e, row.at(in, 0), row.length(), idx, active);
    e.store_states(states, n);
    if (active && e.writes_mode() && row.walks()) {
        mode_tag[gid] = PMX_MODE_ABSORBING;                    // mod.rs:130-132
        mode_index[gid] = idx;
    }
}

template <class Engine>
__global__ void __launch_bounds__(Engine::kThreads, Engine::kMinWavesDriver)
    squeeze_kernel(const DevConfig d, const uint32_t *__restrict__ consts, uint64_t *__restrict__ states,
                   uint32_t *__restrict__ mode_tag, uint32_t *__restrict__ mode_index, uint64_t *__restrict__ out,
                   size_t out_len, size_t n) {
    static_assert(!Engine::kWaveUniformOnly, "this engine's permutation cannot run under the per-lane EXEC masks of squeeze_elements");
    Engine e(d, consts);
    const size_t gid = Engine::unit();
    const bool active = gid < n;
    e.load_states(states, n);
    uint32_t idx = 0;
    bool need = true;                                          // Absorbing -> permute, start at 0 (mod.rs:324-328)
    if (active && mode_tag[gid] == PMX_MODE_SQUEEZING) {       // mod.rs:330-336
        idx = mode_index[gid];
        if (idx > e.c.rate) idx = e.c.rate;                    // see absorb_kernel
        need = idx == e.c.rate;
        if (need) idx = 0;
    }
    idx = squeeze_elements(e, out + (active ? gid : 0) * out_len * 4, out_len, idx, need, active);
    e.store_states(states, n);
    if (active && e.writes_mode()) {
        mode_tag[gid] = PMX_MODE_SQUEEZING;                    // mod.rs:162-164
        mode_index[gid] = idx;
    }
}

// The absorb / squeeze driver of the wide states as PASSES (pmx_sponge_plan.hpp; mod.rs:121-182, 232-254, 321-341).
// A sponge's call alternates data movement and permutations; pass p is "the sponge's own p-th permutation, then whatever
// follows it up to the next one".  Data movement = input elements added into the rate portion (field addition on the ABI
// residues, mod.rs:128,143) or rate elements copied out (mod.rs:159-170).  It never indexes registers dynamically:
//   - a chunk IN FRONT of a permutation is added as the state comes into the permuting kernel's registers (AbsorbAdjust);
//   - a chunk right BEHIND a permutation is copied out of the LDS staging of that kernel's store (CopyOut);
//   - a chunk no permutation follows is moved in global memory by the lane that owns the sponge (sponge_walk), which also
//     rewrites the mode words when the call is over for the sponge (mod.rs:130-132, 162-164).
// Until then every step re-derives its share from the sponge's ORIGINAL mode words.
//   sponge_first_kernel    pass 0 over the whole batch in place: walk, then the workgroup permutes if any of its sponges is
//                          due and only those take the result; walk on; sponges due again go onto list 1 (one atomic per wave).
//   permute_listed_kernel  pass p >= 1: the permutation of the sponges on list p, then walk on -> list p + 1 or finished.
// Both run the permutation wave-uniform on the permutation engine of the width (the matrix-core one at t = 7..9) with
// nothing per-sponge live across it but one ballot; and from the second permutation on a batch in mixed modes costs the
// permutations the reference would execute, not max-over-a-wave of them.
template <bool SQUEEZE, class Row>
__device__ __forceinline__ bool sponge_walk(const Rounds &c, const uint32_t *__restrict__ p32, uint64_t *__restrict__ states, uint32_t *__restrict__ mode_tag,
                                            uint32_t *__restrict__ mode_index, uint64_t *__restrict__ io, const Row &rw, size_t sponge, bool active,
                                            uint32_t pass, uint32_t call_last_pass, bool first_move_done = false) {
    if (!active || !rw.walks()) return false;   // (an empty ragged row: the sponge is not touched at all)
    const uint32_t tag = mode_tag[sponge], index = mode_index[sponge], t_all = c.rate + c.capacity;
    const uint32_t len = (uint32_t)rw.length();
    for (uint32_t q = pass;; ++q) {
        const SpongePass sp = SQUEEZE ? squeeze_pass(tag, index, len, c.rate, c.capacity, q) : absorb_pass(tag, index, len, c.rate, c.capacity, q);
        // absorb: the chunk in front of a permutation is added by the kernel that permutes, as the state comes into its
        // registers (AbsorbAdjust) - only a chunk no permutation follows is added here, in memory
        if (!SQUEEZE && sp.permute) return true;
        uint32_t *st = reinterpret_cast<uint32_t *>(states + (sponge * t_all + sp.state_pos) * 4);
        uint32_t *row = reinterpret_cast<uint32_t *>(rw.at(io, sp.first));
        // squeeze: the chunk right behind a permutation was copied out of the LDS staging by the kernel that permuted (CopyOut)
        const uint32_t todo = (SQUEEZE && first_move_done && q == pass) ? 0 : sp.count;
        for (uint32_t j = 0; j < todo; ++j) {
            if constexpr (SQUEEZE) {
                abi_store(row + 8 * j, abi_load(st + 8 * j));
            } else {
                // state[capacity + i] += element: both fully reduced residues, the sum reduced exactly (no multiplication)
                abi_store(st + 8 * j, abi_add_mod(abi_load(st + 8 * j), abi_load(row + 8 * j), p32));
            }
        }
        if (sp.permute) return true;   // its permutation q follows: only q == pass can get here (permutations are numbered consecutively)
        if (rw.ends(q, call_last_pass, sp)) {   // the call is over for this sponge
            mode_tag[sponge] = SQUEEZE ? PMX_MODE_SQUEEZING : PMX_MODE_ABSORBING;
            mode_index[sponge] = sp.end_index;
            return false;
        }
    }
}

// the sponges of this wave whose next permutation is due go onto the next pass's list, in lane order (one atomic per wave)
__device__ __forceinline__ void sponge_queue(bool queued, size_t sponge, uint32_t *__restrict__ list_next, uint32_t *__restrict__ count_next) {
    const uint64_t want = __builtin_amdgcn_ballot_w64(queued);
    if (want) {
        const uint32_t lane = threadIdx.x & 63, leader = (uint32_t)__builtin_ctzll(want);
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(count_next, (uint32_t)__builtin_popcountll(want));
        base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
        if (queued) list_next[base + (uint32_t)__builtin_popcountll(want & ((1ull << lane) - 1))] = (uint32_t)sponge;
    }
}

// Pass 0 over the whole batch, in place: most calls send (nearly) every sponge through a first permutation - any absorb that
// overflows the rate, any squeeze of an absorbing sponge - so it is not worth a list; a workgroup none of whose sponges
// permutes leaves early, and the moves in front of the permutation hide under the other workgroups' arithmetic.
template <class Engine, bool SQUEEZE, class Rows>
__global__ void __launch_bounds__(Engine::kThreads, Engine::kMinWaves)
    sponge_first_kernel(const DevConfig d, const uint32_t *__restrict__ consts, uint64_t *__restrict__ states,
                        uint32_t *__restrict__ mode_tag, uint32_t *__restrict__ mode_index, uint64_t *__restrict__ io, Rows rows, size_t n,
                        uint32_t last_pass, uint32_t *__restrict__ list1, uint32_t *__restrict__ count1) {
    const size_t gid = (size_t)blockIdx.x * Engine::kThreads + threadIdx.x;
    const uint32_t *p32 = consts + d.io_offset + kIoP32;   // the modulus as 8 x 32-bit limbs (wave-uniform: scalar loads)
    const typename Rows::Row row = rows.row(gid, gid < n);
    const bool due = sponge_walk<SQUEEZE>(d.rounds, p32, states, mode_tag, mode_index, io, row, gid, gid < n, 0, last_pass);
    const uint64_t due_mask = __builtin_amdgcn_ballot_w64(due);       // wave-uniform: the only thing live across the permutation
    {   // workgroup vote through the first word of the DYNAMIC LDS (free until the engine is built): __syncthreads_or keeps a static
        // word of its own, which would come on top of the engine's dynamic LDS (72 KiB at t = 9: two workgroups per CU)
        uint32_t *flag = reinterpret_cast<uint32_t *>(pmx_lds);
        if (threadIdx.x == 0) *flag = 0;
        __syncthreads();
        if (due_mask != 0 && (threadIdx.x & 63) == 0) *flag = 1;   // (every writer writes the same value)
        __syncthreads();
        const bool any = *flag != 0;
        __syncthreads();
        if (!any) return;
    }
    {
        Engine e(d, consts);
        typename Engine::AbsorbAdjust add{nullptr, p32, 0, 0};
        if (!SQUEEZE && due) {   // the chunk in front of this sponge's permutation 0 (none if its mode asks for the permutation up front)
            const SpongePass sp = absorb_pass(mode_tag[gid], mode_index[gid], (uint32_t)row.length(), d.rounds.rate, d.rounds.capacity, 0);
            add.row = reinterpret_cast<const uint32_t *>(row.at(io, sp.first));
            add.pos = sp.state_pos;
            add.count = sp.count;
        }
        e.load_states(states, n, add);
        e.permute(0, e.c.rate + e.c.capacity);   // (run-time width: see permute_kernel)
        typename Engine::CopyOut out{nullptr, 0, 0};
        if (SQUEEZE && ((due_mask >> (threadIdx.x & 63)) & 1)) {   // the chunk right behind permutation 0
            const SpongePass sp = squeeze_pass(mode_tag[gid], mode_index[gid], (uint32_t)row.length(), d.rounds.rate, d.rounds.capacity, 1);
            out.row = reinterpret_cast<uint32_t *>(row.at(io, sp.first));
            out.pos = sp.state_pos;
            out.count = sp.count;
        }
        e.store_states_where(states, n, due_mask, out);
    }
    const bool mine_due = (due_mask >> (threadIdx.x & 63)) & 1;
    // (the wave's span was written by other lanes of the SAME wave after a workgroup barrier: make it visible to this lane's loads)
    __threadfence_block();
    const typename Rows::Row row_after = rows.refetch(gid, gid < n);
    const bool again = sponge_walk<SQUEEZE>(d.rounds, p32, states, mode_tag, mode_index, io, row_after, gid, mine_due, 1, last_pass, true);
    sponge_queue(again, gid, list1, count1);
}

template <class Engine, bool SQUEEZE, class Rows>
__global__ void __launch_bounds__(Engine::kThreads, Engine::kMinWaves)
    permute_listed_kernel(const DevConfig d, const uint32_t *__restrict__ consts, uint64_t *__restrict__ states,
                          uint32_t *__restrict__ mode_tag, uint32_t *__restrict__ mode_index, uint64_t *__restrict__ io, Rows rows,
                          uint32_t pass, uint32_t last_pass, const uint32_t *__restrict__ list, const uint32_t *__restrict__ list_count,
                          uint32_t *__restrict__ list_next, uint32_t *__restrict__ count_next) {
    // The count and the list were produced by the atomics and stores of the PREVIOUS launch, at addresses an earlier launch of
    // this very call has already read (the two lists alternate, the counters share a cache line): they are read with
    // device-scope atomic loads, past the scalar cache and the vector L1, which a back-to-back launch does not always
    // find invalidated (tools/soak.py: calls with two or more listed passes lost sponges to a stale zero count).
    const uint32_t count = __hip_atomic_load(const_cast<uint32_t *>(list_count), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((size_t)blockIdx.x * Engine::kThreads >= count) return;      // (the grid is sized for the whole batch)
    const size_t slot = (size_t)blockIdx.x * Engine::kThreads + threadIdx.x;
    const bool active = slot < count;
    const size_t sponge = __hip_atomic_load(const_cast<uint32_t *>(list) + (active ? slot : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const typename Rows::Row row = rows.row(sponge, active);
    {
        Engine e(d, consts);
        uint64_t *mine = states + sponge * (size_t)(e.c.rate + e.c.capacity) * 4;
        const uint32_t *p32 = consts + d.io_offset + kIoP32;
        typename Engine::AbsorbAdjust add{nullptr, p32, 0, 0};
        if (!SQUEEZE && active) {    // the chunk in front of this sponge's permutation `pass`
            const SpongePass sp = absorb_pass(mode_tag[sponge], mode_index[sponge], (uint32_t)row.length(), d.rounds.rate, d.rounds.capacity, pass);
            add.row = reinterpret_cast<const uint32_t *>(row.at(io, sp.first));
            add.pos = sp.state_pos;
            add.count = sp.count;
        }
        e.load_state_at(mine, add);
        e.permute(0, e.c.rate + e.c.capacity);   // (run-time width: see permute_kernel)
        typename Engine::CopyOut out{nullptr, 0, 0};
        if (SQUEEZE && active) {     // the chunk right behind it
            const SpongePass sp = squeeze_pass(mode_tag[sponge], mode_index[sponge], (uint32_t)row.length(), d.rounds.rate, d.rounds.capacity, pass + 1);
            out.row = reinterpret_cast<uint32_t *>(row.at(io, sp.first));
            out.pos = sp.state_pos;
            out.count = sp.count;
        }
        // a batch in ONE mode lists whole waves of consecutive sponges (the start kernel appends a wave's sponges in lane order)
        const uint32_t lane = threadIdx.x & 63;
        const size_t lead = (size_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)sponge) | ((size_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(sponge >> 32)) << 32);
        const uint64_t live = __builtin_amdgcn_ballot_w64(active);
        const bool together = __builtin_amdgcn_ballot_w64(!active || sponge == lead + lane) == ~0ull;
        e.store_state_at(mine, active, together, states + lead * (size_t)(e.c.rate + e.c.capacity) * 4, (uint32_t)__builtin_popcountll(live), out);
    }
    // (written through the wave's LDS region by the lanes of the SAME wave: make it visible to this lane's loads)
    __threadfence_block();
    const typename Rows::Row row_after = rows.refetch(sponge, active);
    const bool again = sponge_walk<SQUEEZE>(d.rounds, consts + d.io_offset + kIoP32, states, mode_tag, mode_index, io, row_after, sponge, active, pass + 1, last_pass, true);
    sponge_queue(again, sponge, list_next, count_next);
}

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
        uint32_t *scratch = nullptr;                     // [counters, padded to 64 words | list A: n | list B: n]
        const size_t head = (passes + 63) / 64 * 64;
        hipError_t e = hipSuccess;
        uint32_t *lists[2] = {nullptr, nullptr};
        if (launches > 1) {                              // a second permutation is possible: its sponges travel on a list
            // (NOT hipMallocAsync / hipFreeAsync: with several contexts - several streams - alive, ROCm 7.0's stream-ordered pool
            // handed out blocks whose earlier use was still in flight; tools/soak.py lost sponges and took a memory fault that way)
            e = provider.get(provider.owner, st, (head + 2 * n) * 4, &scratch);
            if (e != hipSuccess) return e;
            // (from here on every way out passes provider.done: the block is released by the event recorded there)
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
        if (scratch && provider.done) provider.done(provider.owner, st, scratch);   // behind the last launch that reads the lists
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

#if PMX_TU == 99
// ---- tuning aid (Makefile target asm1): ONE kernel of one window engine, for reading its ISA and register report in seconds ----------
#if !defined(PMX_ONE_T) || !defined(PMX_ONE_ALPHA)
#error "PMX_TU = 99 (make asm1) names its engine with -DPMX_ONE_T=<width> -DPMX_ONE_ALPHA=<5 | 0>"
#endif
#ifdef PMX_ONE_P1   // (make asm1 ... EXTRA=-DPMX_ONE_P1: the engine of a modulus that is 1 mod 2^29)
#define PMX_ONE_ENGINE HybridEngineP1<PMX_ONE_T, PMX_ONE_ALPHA>
#else
#define PMX_ONE_ENGINE HybridEngine<PMX_ONE_T, PMX_ONE_ALPHA>
#endif
template __global__ void permute_kernel<PMX_ONE_ENGINE>(const DevConfig, const uint32_t *__restrict__, uint64_t *__restrict__, size_t);
#ifdef PMX_ONE_GRIND    // (make asm1 ... EXTRA=-DPMX_ONE_GRIND: the grind kernel of the same engine as well)
template __global__ void grind_kernel<PMX_ONE_ENGINE>(const DevConfig, const uint32_t *__restrict__, const uint64_t *__restrict__, uint32_t, uint32_t,
                                                                                uint64_t, size_t, uint64_t *__restrict__);
#endif
#ifdef PMX_ONE_MATRIX   // (make asm1 ... EXTRA=-DPMX_ONE_MATRIX: the hash kernel of the same engine and its strided twin as well)
template __global__ void hash_kernel<PMX_ONE_ENGINE>(const DevConfig, const uint32_t *__restrict__, const uint64_t *__restrict__, size_t, uint64_t *__restrict__,
                                                                               size_t, size_t);
template __global__ void hash_strided_kernel<PMX_ONE_ENGINE>(const DevConfig, const uint32_t *__restrict__, const uint64_t *__restrict__, size_t, size_t, size_t,
                                                                                       uint64_t *__restrict__, size_t, size_t);
#endif
#ifdef PMX_ONE_RAGGED   // (make asm1 ... EXTRA=-DPMX_ONE_RAGGED: the two ragged pass kernels of the same engine as well)
hipError_t one_ragged(const DevConfig &c, uint64_t *s, uint32_t *tg, uint32_t *ix, uint64_t *io, const uint64_t *o, size_t n, const PassScratch &p) {
    return Launch<PMX_ONE_ENGINE>::template sponge_passes<false>(c, PMX_ONE_T, s, tg, ix, io, RowsRagged{io, o, 8}, n, 0, p);
}
#endif
#elif PMX_TU != 0
// ---- window engines of this translation unit ------------------------------------------------------------------------
constexpr bool kTuP1 = PMX_TU >= 5;
constexpr int kTuPart = kTuP1 ? PMX_TU - 4 : PMX_TU;
constexpr int kTuAlpha = (kTuPart == 1 || kTuPart == 3) ? 5 : 0;
constexpr bool kTuWide = kTuPart >= 3;
template <int T>
using TuEngine = std::conditional_t<kTuP1, HybridEngineP1<T, kTuAlpha>, HybridEngine<T, kTuAlpha>>;
template <>
const EngineOps *window_ops<kTuAlpha, kTuWide, kTuP1>(uint32_t t) {
    const EngineOps *ops = nullptr;
    static_for<(kTuWide ? 7 : 3), (kTuWide ? 10 : 7)>([&](auto width) {
        if (t == (uint32_t)width) ops = &engine_ops<TuEngine<decltype(width)::value>>();
    });
    return ops;
}

#else  // PMX_TU == 0
// ---- public launchers -------------------------------------------------------------------------------------------------
template <> const EngineOps *window_ops<5, false, false>(uint32_t t);
template <> const EngineOps *window_ops<5, true, false>(uint32_t t);
template <> const EngineOps *window_ops<0, false, false>(uint32_t t);
template <> const EngineOps *window_ops<0, true, false>(uint32_t t);
template <> const EngineOps *window_ops<5, false, true>(uint32_t t);
template <> const EngineOps *window_ops<5, true, true>(uint32_t t);
template <> const EngineOps *window_ops<0, false, true>(uint32_t t);
template <> const EngineOps *window_ops<0, true, true>(uint32_t t);

// the quad engine's table exists (t = 3, optimised schedule) and fits LDS; the lane of each element is fixed by the
// split only where elements are addressed through capacity / rate (quad_shape below)
static bool quad_table(const DevConfig &c, uint32_t t) {
    return t == 3 && c.has_opt && (size_t)c.rounds.total_rounds * 3 * kCoopElems * kFeStride * 4 <= (size_t)c.max_lds_bytes;
}
static bool quad_shape(const DevConfig &c, uint32_t t) { return quad_table(c, t) && c.rounds.capacity == 1 && c.rounds.rate == 2; }

// Small batches are latency: the quad engine up to this many states / rows / sponges / compressions (one dependent chain of 32 k
// instead of 55 k instructions: 0.066 ms up to 4096 states, 0.078 at 2^14, 0.132 at 2^15; above, the one-lane-per-state engine fills the
// chip better - profiles/r05/v_ab_t3_engine_threshold_32769.txt, w_ab_quad_kernels_up_to_16384_only_not_kept.txt).
static constexpr size_t kQuadMaxUnits = 32768;

// the window engine of the config and width (the modulus' and the exponent's part of the family, then the width's), if the config has its
// tables and its LDS fits the device.  A modulus that is 1 mod 2^29 (pmx_prepare.hpp records it: Prepared::unit_low_limb; here it is read off
// the limbs the kernels get) takes the engines with the complemented quotient digits, every other modulus the generic step.
template <bool P1>
static const EngineOps *window_engine_of(const DevConfig &c, uint32_t t) {
    return c.rounds.alpha == 5 ? (t <= 6 ? window_ops<5, false, P1>(t) : window_ops<5, true, P1>(t))
                               : (t <= 6 ? window_ops<0, false, P1>(t) : window_ops<0, true, P1>(t));
}
static const EngineOps *window_engine(const DevConfig &c, uint32_t t) {
    if (!c.has_opt || !c.mfma_dense || t < (uint32_t)PMX_MFMA_MIN_T || t > (uint32_t)PMX_MFMA_MAX_T) return nullptr;
    const EngineOps *w = field_unit_low_limb(c.field.p) ? window_engine_of<true>(c, t) : window_engine_of<false>(c, t);
    return w && w->lds_bytes(c, t) <= (size_t)c.max_lds_bytes ? w : nullptr;
}
// the quad or run-time-width engine of the config's exponent
template <template <int> class Engine>
static const EngineOps *by_alpha(const DevConfig &c) {
    return c.rounds.alpha == 5 ? &engine_ops<Engine<5>>() : c.rounds.alpha == 17 ? &engine_ops<Engine<17>>() : &engine_ops<Engine<0>>();
}

// Engine choice (three engines, one per regime):
//   QuadEngine     t = 3, at most 32768 units: one state per quad of lanes - the call is one permutation's latency
//   HybridEngine   t = 3 .. 9, configs that have the window tables (DevConfig::mfma_dense: the optimised schedule exists, at least two
//                  full rounds, the window algebra meets no zero - every config of the reference's tables, any modulus): alpha = 5
//                  specialised, any other exponent on the generic S-box; absorb / squeeze as passes
//   LdsEngine      everything else (t = 2, t >= 10, no partial section, a zero in the algebra): run-time width, the reference's dense schedule
// alpha 5 and 17 have dedicated addition chains in the quad and run-time-width engines, other exponents share the generic S-box.
// The ONLY place that decides it: every launcher below and describe_launch (pmx_ctx_engine_info) go through the table returned here.
// nullptr: `op` is none of PMX_OP_*.
static const EngineOps *select_engine(const DevConfig &c, uint32_t t, int op, size_t n) {
    bool quad;
    switch (op) {
        case PMX_OP_PERMUTE: quad = quad_table(c, t); break;
        case PMX_OP_HASH:
        case PMX_OP_ABSORB:
        case PMX_OP_SQUEEZE:
        // (the split (rate 3, capacity 0) of the same width takes the one-lane-per-state engine at every tree level)
        case PMX_OP_COMPRESS:
        // (a chunk of n candidates addresses the state through capacity + index like a compression)
        case PMX_OP_GRIND: quad = quad_shape(c, t); break;
        default: return nullptr;
    }
    if (quad && n <= kQuadMaxUnits) return by_alpha<QuadEngine>(c);
    if (const EngineOps *w = window_engine(c, t)) return w;
    return by_alpha<LdsEngine>(c);
}

hipError_t launch_permute(const DevConfig &c, uint32_t t, uint64_t *states, size_t n, hipStream_t st) {
    return select_engine(c, t, PMX_OP_PERMUTE, n)->permute(c, t, states, n, st);
}
hipError_t launch_hash(const DevConfig &c, uint32_t t, const uint64_t *in, size_t in_len, uint64_t *out, size_t out_len,
                       size_t n, hipStream_t st) {
    return select_engine(c, t, PMX_OP_HASH, n)->hash(c, t, in, in_len, out, out_len, n, st);
}
// the rows of a matrix (hash_strided_kernel): a hash like any other to the engine choice
hipError_t launch_hash_strided(const DevConfig &c, uint32_t t, const uint64_t *in, size_t in_len, size_t row_stride, size_t elem_stride,
                               uint64_t *out, size_t out_len, size_t n, hipStream_t st) {
    return select_engine(c, t, PMX_OP_HASH, n)->hash_strided(c, t, in, in_len, row_stride, elem_stride, out, out_len, n, st);
}
hipError_t launch_compress(const DevConfig &c, uint32_t t, const uint64_t *in, uint64_t *out, size_t n, hipStream_t st) {
    return select_engine(c, t, PMX_OP_COMPRESS, n)->compress(c, t, in, out, n, st);
}
// arity 2 IS the 2-to-1 launch (the quad engine included, which needs rate 2 and so never meets a wider row); a wider row goes to the
// compress_ary kernel of the engine the same choice names.  (An arity beyond the rate would index past the state: refused here too.)
hipError_t launch_compress_ary(const DevConfig &c, uint32_t t, const uint64_t *in, uint64_t *out, uint32_t arity, size_t n, hipStream_t st) {
    if (arity < 2 || arity > c.rounds.rate) return hipErrorInvalidValue;
    if (arity == 2) return launch_compress(c, t, in, out, n, st);
    return select_engine(c, t, PMX_OP_COMPRESS, n)->compress_ary(c, t, in, out, arity, n, st);
}
// One tree level of n_children nodes, any number of them (pmx_merkle_ragged*): ceil(n_children / arity) parents in ONE launch on the engine
// the choice names for that many parents, the quad engine included.  A level that divides by the arity is launch_compress_ary, launch
// for launch; only a level with a short last row runs the bounded twin, at arity 2 too - never a second launch for the odd child.
hipError_t launch_compress_level(const DevConfig &c, uint32_t t, const uint64_t *in, uint64_t *out, uint32_t arity, size_t n_children,
                                 hipStream_t st) {
    if (arity < 2 || arity > c.rounds.rate || n_children == 0) return hipErrorInvalidValue;
    const size_t n = n_children / arity + (n_children % arity ? 1 : 0);
    if (n_children % arity == 0) return launch_compress_ary(c, t, in, out, arity, n, st);
    return select_engine(c, t, PMX_OP_COMPRESS, n)->compress_ary_bounded(c, t, in, out, arity, n_children, n, st);
}
// One chunk of a grinding search (grind_kernel): the n nonces first .. first + n - 1 against the base state at `base`, index < rate;
// *best is lowered to the smallest accepted one.  (An index at or beyond the rate would address past the state: refused here too.)
hipError_t launch_grind(const DevConfig &c, uint32_t t, const uint64_t *base, uint32_t index, uint32_t bits, uint64_t first, size_t n,
                        uint64_t *best, hipStream_t st) {
    if (index >= c.rounds.rate || n == 0 || n > (size_t)0x7fffffff * 64 || first + (uint64_t)(n - 1) < first) return hipErrorInvalidValue;
    return select_engine(c, t, PMX_OP_GRIND, n)->grind(c, t, base, index, bits, first, n, best, st);
}
hipError_t launch_absorb(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index,
                         const uint64_t *in, size_t in_len, size_t n, hipStream_t st, const PassScratch &scratch) {
    return select_engine(c, t, PMX_OP_ABSORB, n)->absorb(c, t, states, tag, index, in, in_len, n, st, scratch);
}
hipError_t launch_squeeze(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index,
                          uint64_t *out, size_t out_len, size_t n, hipStream_t st, const PassScratch &scratch) {
    return select_engine(c, t, PMX_OP_SQUEEZE, n)->squeeze(c, t, states, tag, index, out, out_len, n, st, scratch);
}
// ragged rows: an absorb like any other to the engine choice
hipError_t launch_absorb_varlen(const DevConfig &c, uint32_t t, uint64_t *states, uint32_t *tag, uint32_t *index, const uint64_t *in,
                                const uint64_t *offsets, size_t max_len, size_t n, hipStream_t st, const PassScratch &scratch) {
    return select_engine(c, t, PMX_OP_ABSORB, n)->absorb_varlen(c, t, states, tag, index, in, offsets, max_len, n, st, scratch);
}
// per row: new; absorb(row); squeeze_native(out_len) = n fresh sponges (Absorbing{0} and a zero state: all-zero words, mod.rs:219-230) in
// a block of the pass pool, the ragged absorb on them, then the fixed squeeze writing straight into `out`.  (The pass form of the absorb
// costs the permutations the reference executes; a ragged register-resident hash kernel would pay max-over-a-wave of them.)
hipError_t launch_hash_varlen(const DevConfig &c, uint32_t t, const uint64_t *in, const uint64_t *offsets, size_t max_len, uint64_t *out,
                              size_t out_len, size_t n, hipStream_t st, const PassScratch &scratch) {
    const size_t st_bytes = n * t * 32, words = (n + 3) / 4 * 4;   // (the mode words start 16-byte aligned)
    uint32_t *block = nullptr;
    hipError_t e = scratch.get(scratch.owner, st, st_bytes + 2 * words * 4, &block);
    if (e != hipSuccess) return e;
    uint64_t *states = reinterpret_cast<uint64_t *>(block);
    uint32_t *tag = block + st_bytes / 4, *index = tag + words;
    e = hipMemsetAsync(block, 0, st_bytes + 2 * words * 4, st);
    if (e == hipSuccess) e = launch_absorb_varlen(c, t, states, tag, index, in, offsets, max_len, n, st, scratch);
    if (e == hipSuccess) e = launch_squeeze(c, t, states, tag, index, out, out_len, n, st, scratch);
    scratch.done(scratch.owner, st, block);   // behind the squeeze, the last launch that reads the block
    return e;
}

// ---- pmx_ctx_engine_info: the engine the launcher of `op` selects, describing instead of launching --------------------------
hipError_t describe_launch(const DevConfig &c, uint32_t t, int op, size_t n, size_t len, EngineInfo *o) {
    std::memset(o, 0, sizeof *o);
    o->width = (int)t;
    const EngineOps *engine = select_engine(c, t, op, n);
    if (!engine) return hipErrorInvalidValue;
    engine->describe(c, t, op, len, o);
    return hipSuccess;
}

// ---- authentication paths (pmx_merkle_verify_paths_dev) --------------------------------------------------------------
// Pure data movement: four lanes per path, one 16-byte quarter of the 64-byte pair each.
__global__ void __launch_bounds__(256) path_pairs_kernel(const uint4 *__restrict__ cur, const uint4 *__restrict__ paths,
                                                         const uint64_t *__restrict__ indices, size_t depth, size_t level,
                                                         uint4 *__restrict__ pairs, size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, i = gid >> 2;
    if (i >= k) return;
    const uint32_t quarter = gid & 3, half = quarter & 1;
    const bool right = (indices[i] >> level) & 1;          // the running node is the right child at this level
    const bool from_cur = (quarter >> 1) == (right ? 1u : 0u);
    pairs[gid] = from_cur ? cur[i * 2 + half] : paths[(i * depth + level) * 2 + half];
}

// the same for a tree of any arity (pmx_merkle_ary_verify_paths_dev): 2 arity lanes per path, one 16-byte quarter of a child each.
// Row i of `rows` is the arity children of path i's parent at `level`: the running node at digit (index / arity^level) % arity, the
// arity - 1 siblings of paths[i][level] in child order around it.  pow = arity^level (the caller's; >= 1).  The digit is below the
// arity whatever the index holds, so an index that names no leaf still reads inside the arrays.
__global__ void __launch_bounds__(256) path_children_kernel(const uint4 *__restrict__ cur, const uint4 *__restrict__ paths,
                                                            const uint64_t *__restrict__ indices, size_t depth, size_t level, uint64_t pow,
                                                            uint32_t arity, uint4 *__restrict__ rows, size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, per = 2 * (size_t)arity, i = gid / per;
    if (i >= k) return;
    const uint32_t quarter = (uint32_t)(gid - i * per), child = quarter >> 1, half = quarter & 1;
    const uint32_t digit = (uint32_t)((indices[i] / pow) % arity);
    const uint32_t sibling = child < digit ? child : child - 1;   // the running node's own slot is left out of the path
    rows[gid] = child == digit ? cur[i * 2 + half] : paths[((i * depth + level) * (arity - 1) + sibling) * 2 + half];
}

// The opening itself on the device (pmx_merkle_ary_paths_dev): from the node array (leaves, then every level, root last) to paths
// [k][depth][arity - 1][4], one 16-byte quarter per lane.  Device-resident indices are not validated by the host: an index that names
// no leaf gets an all-zero path, and nothing outside the node array is read.
__global__ void __launch_bounds__(256) paths_gather_kernel(const uint4 *__restrict__ nodes, uint64_t n_leaves, uint32_t arity, size_t depth,
                                                           const uint64_t *__restrict__ indices, uint4 *__restrict__ paths, size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, per_level = 2 * (size_t)(arity - 1), per = depth * per_level, i = gid / per;
    if (i >= k) return;
    const size_t rest = gid - i * per, level = rest / per_level;
    const uint32_t quarter = (uint32_t)(rest - level * per_level), sibling = quarter >> 1, half = quarter & 1;
    uint64_t idx = indices[i], first = 0, width = n_leaves;   // the running node's index in its level, the level's first node, its width
    if (idx >= n_leaves) {
        paths[gid] = make_uint4(0, 0, 0, 0);
        return;
    }
    for (size_t l = 0; l < level; ++l) {
        first += width;
        width /= arity;
        idx /= arity;
    }
    const uint32_t digit = (uint32_t)(idx % arity);
    const uint32_t child = sibling < digit ? sibling : sibling + 1;
    paths[gid] = nodes[(first + (idx - digit) + child) * 2 + half];
}

// ok[i] = the running node equals the root and indices[i] < limit, the number of leaves a tree of this depth has (2^depth, arity^depth)
__global__ void __launch_bounds__(256) path_check_kernel(const uint4 *__restrict__ cur, const uint4 *__restrict__ root,
                                                         const uint64_t *__restrict__ indices, uint64_t limit,
                                                         uint8_t *__restrict__ ok, size_t k) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= k) return;
    const uint4 a = cur[i * 2], b = cur[i * 2 + 1], ra = root[0], rb = root[1];
    const bool same = a.x == ra.x && a.y == ra.y && a.z == ra.z && a.w == ra.w && b.x == rb.x && b.y == rb.y && b.z == rb.z && b.w == rb.w;
    ok[i] = (same && indices[i] < limit) ? 1 : 0;
}

// ---- leaf updates of a resident tree (pmx_merkle_ary_update_dev, pmx_merkle_ary_update) -------------------------------------------
// Pure data movement around launch_compress_ary, like the path kernels above.  The scatter: two lanes per element, one 16-byte half each,
// dst[base + indices[i] / pow] = src[i] if indices[i] < limit.  The leaves go in with pow = 1, base = 0; the parents of level l + 1 with
// pow = arity^(l+1), base = the level's first node (limit = n_leaves both times: index / pow is then below the level's width); the host
// entry's digests go to explicit slots of its packed rows (pow = 1, limit = the slots the level has).  An index at or above the limit
// stores nothing.  Two lanes that store to one element store what their sources hold: equal sources, equal bytes.  pow >= 1.
__global__ void __launch_bounds__(256) node_scatter_kernel(const uint4 *__restrict__ src, const uint64_t *__restrict__ indices, uint64_t pow,
                                                           uint64_t limit, uint64_t base, uint4 *__restrict__ dst, size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, i = gid >> 1;
    if (i >= k) return;
    const uint64_t idx = indices[i];
    if (idx >= limit) return;
    dst[(base + idx / pow) * 2 + (gid & 1)] = src[gid];
}

// The gather: 2 arity lanes per update, one 16-byte half of a child each.  Row i of `rows` is the arity children of update i's parent
// p = indices[i] / pow (pow = arity^(l+1)) out of level l, whose first node is `first`: nodes[first + p * arity ...].  An index that names no
// leaf (>= n_leaves) gathers the row of parent 0 - in range like every other, and its parent is never stored (the scatter above).
__global__ void __launch_bounds__(256) node_children_kernel(const uint4 *__restrict__ nodes, const uint64_t *__restrict__ indices, uint64_t pow,
                                                            uint64_t n_leaves, uint64_t first, uint32_t arity, uint4 *__restrict__ rows,
                                                            size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, per = 2 * (size_t)arity, i = gid / per;
    if (i >= k) return;
    const uint64_t idx = indices[i], p = idx < n_leaves ? idx / pow : 0;
    rows[gid] = nodes[(first + p * arity) * 2 + (gid - i * per)];
}

// ---- trees over any number of leaves (pmx_merkle_ragged*) -------------------------------------------------------------------------------
// Level l + 1 has ceil(M_l / arity) nodes, so a level's width and first row are carried down the levels, not divided out.  Bounded twins of
// paths_gather_kernel and node_children_kernel: a child at or beyond its level's width does not exist - it is four zero words in the
// opening and in the gathered row (the zero a short parent's rate lane holds), and nothing at or beyond the level's end is read.
__global__ void __launch_bounds__(256) paths_gather_ragged_kernel(const uint4 *__restrict__ nodes, uint64_t n_leaves, uint32_t arity, size_t depth,
                                                                  const uint64_t *__restrict__ indices, uint4 *__restrict__ paths, size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, per_level = 2 * (size_t)(arity - 1), per = depth * per_level, i = gid / per;
    if (i >= k) return;
    const size_t rest = gid - i * per, level = rest / per_level;
    const uint32_t quarter = (uint32_t)(rest - level * per_level), sibling = quarter >> 1, half = quarter & 1;
    uint64_t idx = indices[i], first = 0, width = n_leaves;   // the running node's index in its level, the level's first node, its width
    uint4 v = make_uint4(0, 0, 0, 0);
    if (idx < n_leaves) {
        for (size_t l = 0; l < level; ++l) {
            first += width;
            width = width / arity + (width % arity ? 1 : 0);
            idx /= arity;
        }
        const uint32_t digit = (uint32_t)(idx % arity);
        const uint64_t child = (idx - digit) + (sibling < digit ? sibling : sibling + 1);   // in its level
        if (child < width) v = nodes[(first + child) * 2 + half];
    }
    paths[gid] = v;
}

// `width`: the nodes level l has (its first node is `first`); parent p = indices[i] / pow has the children p * arity .. below width
__global__ void __launch_bounds__(256) node_children_bounded_kernel(const uint4 *__restrict__ nodes, const uint64_t *__restrict__ indices,
                                                                    uint64_t pow, uint64_t n_leaves, uint64_t first, uint64_t width,
                                                                    uint32_t arity, uint4 *__restrict__ rows, size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, per = 2 * (size_t)arity, i = gid / per;
    if (i >= k) return;
    const uint32_t quarter = (uint32_t)(gid - i * per), half = quarter & 1;
    const uint64_t idx = indices[i], p = idx < n_leaves ? idx / pow : 0, child = p * arity + (quarter >> 1);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (child < width) v = nodes[(first + child) * 2 + half];
    rows[gid] = v;
}

// THE launch of a data-movement kernel, whichever: one lane per 16-byte piece it writes (path_check_kernel: per path), 256 lanes a
// workgroup, no LDS.  The elements of the callers' uint64_t arrays reach the kernels as their 16-byte halves (u4).
static const uint4 *u4(const uint64_t *p) { return reinterpret_cast<const uint4 *>(p); }
static uint4 *u4(uint64_t *p) { return reinterpret_cast<uint4 *>(p); }
template <class K, class... A>
static hipError_t plain(K kernel, size_t lanes, hipStream_t st, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, args...);
    return hipGetLastError();
}

hipError_t launch_paths_gather_ragged(const uint64_t *nodes, size_t n_leaves, uint32_t arity, size_t depth, const uint64_t *indices,
                                      uint64_t *paths, size_t k, hipStream_t st) {
    return plain(paths_gather_ragged_kernel, k * depth * 2 * (arity - 1), st, u4(nodes), n_leaves, arity, depth, indices, u4(paths), k);
}
hipError_t launch_node_children_bounded(const uint64_t *nodes, const uint64_t *indices, uint64_t pow, uint64_t n_leaves, uint64_t first,
                                        uint64_t width, uint32_t arity, uint64_t *rows, size_t k, hipStream_t st) {
    return plain(node_children_bounded_kernel, k * 2 * arity, st, u4(nodes), indices, pow, n_leaves, first, width, arity, u4(rows), k);
}

hipError_t launch_node_scatter(const uint64_t *src, const uint64_t *indices, uint64_t pow, uint64_t limit, uint64_t base, uint64_t *dst,
                               size_t k, hipStream_t st) {
    return plain(node_scatter_kernel, k * 2, st, u4(src), indices, pow, limit, base, u4(dst), k);
}
hipError_t launch_node_children(const uint64_t *nodes, const uint64_t *indices, uint64_t pow, uint64_t n_leaves, uint64_t first, uint32_t arity,
                                uint64_t *rows, size_t k, hipStream_t st) {
    return plain(node_children_kernel, k * 2 * arity, st, u4(nodes), indices, pow, n_leaves, first, arity, u4(rows), k);
}

// ---- fixed-depth trees (pmx_merkle_fixed*, pmx_merkle_frontier_append) ----------------------------------------------------------------
// Pure data movement around the compression launches, driven by a list the host built (pmx_merkle_frontier.hpp): entry i is the pair
// (list[2 i], list[2 i + 1]) = (destination element, source element) of `elems`, two lanes per entry, one 16-byte half each.  It lays the
// uploaded frontier nodes and the default digests into the levels' rows before the walk and collects the new frontier and the root behind
// it.  Sources and destinations of one launch never overlap (the host's lists read what was uploaded or computed and write elsewhere),
// but they lie in one array: no __restrict__ on it.
__global__ void __launch_bounds__(256) node_place_kernel(uint4 *elems, const uint64_t *__restrict__ list, size_t k) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, i = gid >> 1;
    if (i >= k) return;
    elems[list[2 * i] * 2 + (gid & 1)] = elems[list[2 * i + 1] * 2 + (gid & 1)];
}
hipError_t launch_node_place(uint64_t *elems, const uint64_t *list, size_t k, hipStream_t st) {
    return plain(node_place_kernel, k * 2, st, u4(elems), list, k);
}

hipError_t launch_path_pairs(const uint64_t *cur, const uint64_t *paths, const uint64_t *indices, size_t depth, size_t level,
                             uint64_t *pairs, size_t k, hipStream_t st) {
    return plain(path_pairs_kernel, k * 4, st, u4(cur), u4(paths), indices, depth, level, u4(pairs), k);
}
hipError_t launch_path_children(const uint64_t *cur, const uint64_t *paths, const uint64_t *indices, size_t depth, size_t level, uint64_t pow,
                                uint32_t arity, uint64_t *rows, size_t k, hipStream_t st) {
    return plain(path_children_kernel, k * 2 * arity, st, u4(cur), u4(paths), indices, depth, level, pow, arity, u4(rows), k);
}
hipError_t launch_paths_gather(const uint64_t *nodes, size_t n_leaves, uint32_t arity, size_t depth, const uint64_t *indices, uint64_t *paths,
                               size_t k, hipStream_t st) {
    return plain(paths_gather_kernel, k * depth * 2 * (arity - 1), st, u4(nodes), n_leaves, arity, depth, indices, u4(paths), k);
}
hipError_t launch_path_check(const uint64_t *cur, const uint64_t *root, const uint64_t *indices, uint64_t limit, uint8_t *ok,
                             size_t k, hipStream_t st) {
    return plain(path_check_kernel, k, st, u4(cur), u4(root), indices, limit, ok, k);
}
#endif  // PMX_TU

}  // namespace pmx

