// The window engines (pmx_engines.hpp: HybridEngine, HybridEngineP1) with their kernels and launchers: one part of the family per
// compilation, named by -DPMX_TU=1 .. 8 (the Makefile compiles this file eight times, in parallel).  PMX_TU = 1 / 3 hold the engines for
// alpha = 5 (widths up to 6 / from 7), PMX_TU = 2 / 4 the same for the generic S-box (each width x 7 kernels - by far the longest
// compile), PMX_TU = 5 .. 8 those four for a modulus that is 1 mod 2^29.  pmx_device.hip declares the eight lookups and chooses.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pmx_engine_launch.hpp"
#include "pmx_engines.hpp"
#include "pmx_field.hpp"

#if !defined(PMX_TU) || PMX_TU < 1 || PMX_TU > 8
#error "pmx_device_window.hip is compiled with -DPMX_TU=<1 .. 8>, the part of the window engines it holds"
#endif

namespace pmx {

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

}  // namespace pmx
