// CPU restatement of the absorb side of the pass driver with variable-length rows (test infrastructure, not a product path):
// the walk of sponge_walk / sponge_first_kernel / permute_listed_kernel in sponge_amd/csrc/pmx_kernels.hpp, over ONE sponge, built on
// the plan of pmx_sponge_plan.hpp compiled for the host - absorb_pass, and the helpers the ragged kernels use for a row's length, the
// empty-row rule and the end of a sponge's walk at its own last pass.  The permutation is the caller's (tests/test_varlen_plan.py: the C oracle), so the
// test sees the data moved and the permutations performed, in order.
//
// Build: g++ -O1 -std=c++17 -fPIC -shared -Wno-unknown-pragmas -DPMX_HOSTCHECK -I sponge_amd/csrc tests/varlen_plan/varlen_walk.cpp -o <lib>
#include <cstdint>
#include <cstring>

#include "../../include/poseidon_mi355x.h"
#include "pmx_sponge_plan.hpp"

using namespace pmx;

typedef void (*permute_fn)(uint64_t *state);

static Abi load(const uint64_t *p) {
    Abi a;
    std::memcpy(a.w, p, 32);
    return a;
}
static void store(uint64_t *p, const Abi &a) { std::memcpy(p, a.w, 32); }

struct Sponge {
    uint32_t rate, capacity;
    const uint32_t *p32;
    uint64_t *state;       // [t][4]
    uint32_t *tag, *index;
    const uint64_t *row;   // the sponge's row: io + offsets[i] * 4
    uint32_t len, tag0, index0, last, call_last;
    uint32_t steps = 0;    // plan steps walked (every q of every walk)
    bool late = false;     // the walk went past the sponge's own last pass (absorb_last_pass)

    void add(const SpongePass &sp) {
        for (uint32_t j = 0; j < sp.count; ++j)
            store(state + (sp.state_pos + j) * 4, abi_add_mod(load(state + (sp.state_pos + j) * 4), load(row + (sp.first + j) * 4), p32));
    }
    // sponge_walk<false> from pass `pass`: true when the sponge's permutation `pass` is due (its chunk is added by the permuting kernel)
    bool walk(uint32_t pass) {
        for (uint32_t q = pass;; ++q) {
            ++steps;
            const SpongePass sp = absorb_pass(tag0, index0, len, rate, capacity, q);
            if (sp.permute) return true;
            add(sp);
            if (q > last) late = true;
            if (absorb_row_ends(sp, len) || q >= call_last) {   // RowsRagged::Row::ends
                *tag = PMX_MODE_ABSORBING;
                *index = sp.end_index;
                return false;
            }
        }
    }
};

// absorb of row [lo, hi) (clamped to max_len, as the device reads it) on (state, tag, index) the way one call of the ragged pass driver
// runs it: pass 0 (sponge_first_kernel), then one listed pass per further permutation (permute_listed_kernel).  Returns 0, or
// 1 when the sponge would be listed for a pass the call does not launch (its passes come from max_len), 2 when its walk went past its
// own last pass; perms / steps: what it did.
extern "C" int vw_absorb(uint32_t rate, uint32_t capacity, const uint32_t *p32, uint64_t *state, uint32_t *tag, uint32_t *index,
                         const uint64_t *io, uint64_t lo, uint64_t hi, uint32_t max_len, permute_fn permute, uint32_t *perms, uint32_t *steps) {
    *perms = 0;
    *steps = 0;
    const uint32_t len = varlen_row_len(lo, hi, max_len);
    if (!absorb_row_walks(len)) return 0;   // the empty row: nothing is read or written
    const uint32_t call_last = max_len == 0 ? 0 : (uint32_t)(absorb_passes(max_len, rate) - 1);
    Sponge s{rate, capacity, p32, state, tag, index, io + lo * 4, len, *tag, *index, absorb_last_pass(len, rate), call_last};
    bool due = s.walk(0);
    for (uint32_t p = 0; due; ++p) {
        if (p > 0 && p >= call_last) return 1;   // (listed passes are 1 .. call_last - 1)
        s.add(absorb_pass(s.tag0, s.index0, len, rate, capacity, p));   // AbsorbAdjust: the chunk in front of permutation p
        permute(state);
        ++*perms;
        due = s.walk(p + 1);
    }
    *steps = s.steps;
    return s.late ? 2 : 0;
}

// the helpers themselves (pmx_sponge_plan.hpp)
extern "C" uint32_t vw_row_len(uint64_t lo, uint64_t hi, uint32_t max_len) { return varlen_row_len(lo, hi, max_len); }
extern "C" uint32_t vw_last_pass(uint32_t len, uint32_t rate) { return absorb_last_pass(len, rate); }
