// The engine choice and the public launchers (pmx_launch.hpp), with the quad and the run-time-width engine they can name directly
// (pmx_engines.hpp); the window engines are looked up in the eight translation units of pmx_device_window.hip.  Compiled once.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/poseidon_mi355x.h"
#include "pmx_engine_launch.hpp"
#include "pmx_engines.hpp"
#include "pmx_field.hpp"
#include "pmx_internal.hpp"
#include "pmx_launch.hpp"

namespace pmx {

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
    PassLease lease(scratch, st);   // given back behind the squeeze, the last launch that reads the block
    hipError_t e = lease.take(st_bytes + 2 * words * 4);
    if (e != hipSuccess) return e;
    uint32_t *block = lease.block;
    uint64_t *states = reinterpret_cast<uint64_t *>(block);
    uint32_t *tag = block + st_bytes / 4, *index = tag + words;
    e = hipMemsetAsync(block, 0, st_bytes + 2 * words * 4, st);
    if (e == hipSuccess) e = launch_absorb_varlen(c, t, states, tag, index, in, offsets, max_len, n, st, scratch);
    if (e == hipSuccess) e = launch_squeeze(c, t, states, tag, index, out, out_len, n, st, scratch);
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

}  // namespace pmx
