// Tuning aid (Makefile target asm1), never linked: ONE kernel of one window engine, for reading its ISA and register report in seconds.
#include <hip/hip_runtime.h>

#include "pmx_engine_launch.hpp"
#include "pmx_engines.hpp"
#include "pmx_kernels.hpp"

namespace pmx {

#if !defined(PMX_ONE_T) || !defined(PMX_ONE_ALPHA)
#error "pmx_device_one.hip (make asm1) names its engine with -DPMX_ONE_T=<width> -DPMX_ONE_ALPHA=<5 | 0>"
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

}  // namespace pmx
