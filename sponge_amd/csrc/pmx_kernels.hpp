// The kernels of the engines (pmx_engines.hpp): templates on the engine, instantiated where a launcher of that engine is named
// (pmx_engine_launch.hpp), and the row policies and the sponge walk of the absorb / squeeze drivers.
#pragma once
#include <hip/hip_runtime.h>

#include "pmx_engines.hpp"
#include "pmx_field.hpp"
#include "pmx_internal.hpp"
#include "pmx_sponge_plan.hpp"

namespace pmx {

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

}  // namespace pmx
