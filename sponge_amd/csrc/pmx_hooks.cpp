// Host constants of the single-device entries that the test build can replace (include/poseidon_mi355x_testing.h).  Compiled twice
// (Makefile): build/pmx_hooks.o for libposeidon_mi355x.so - the constants and nothing else, no hook symbol, no state - and
// build/pmx_hooks_test.o (-DPMX_TEST_HOOKS) for libposeidon_mi355x_test.so.  (The hooks of the device-group code live in pmx_mgpu.cpp.)
#include <atomic>
#include <cstdint>

#include "../../include/poseidon_mi355x.h"
#include "pmx_ctx.hpp"

namespace pmx {
// Candidates per launch of pmx_sponge_grind (pmx_api.cpp), chosen from the sweep of profiles/grind/README.md.
static constexpr uint64_t kGrindChunk = (uint64_t)1 << 21;
}  // namespace pmx

#ifdef PMX_TEST_HOOKS
static std::atomic<uint64_t> g_grind_chunk{0};   // 0: the product's
extern "C" int pmx_test_grind_chunk(uint64_t candidates) {
    g_grind_chunk.store(candidates);
    return PMX_OK;
}
uint64_t pmx::grind_chunk() {
    const uint64_t set = g_grind_chunk.load();
    return set ? set : kGrindChunk;
}
#else
uint64_t pmx::grind_chunk() { return kGrindChunk; }
#endif
