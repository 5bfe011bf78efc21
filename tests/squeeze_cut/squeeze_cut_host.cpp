// The device-side pieces of squeeze_bytes / squeeze_bits compiled for the host (test infrastructure, not a product path):
// abi_to_canonical of sponge_amd/csrc/pmx_field.hpp - ABI residue -> canonical integer, what the conversion kernels of pmx_convert.hip
// run per element - and the position arithmetic of pmx_squeeze_cut.hpp.  tests/test_squeeze_cut.py compares both with Python integers.
//
// Build: g++ -O1 -std=c++17 -fPIC -shared -Wno-unknown-pragmas -DPMX_HOSTCHECK -I sponge_amd/csrc tests/squeeze_cut/squeeze_cut_host.cpp -o <lib>
#include <cstdint>
#include <cstring>

#include "pmx_squeeze_cut.hpp"

namespace pmx {
void hostcheck_track(int, const Fe &, const FieldRt &) {}
void hostcheck_below_2_256(const Fe &) {}
}  // namespace pmx

using namespace pmx;

// p29: the modulus as 9 x 29-bit limbs, pinv = -p^-1 mod 2^29, p32: the modulus as 8 x 32-bit words (the only part of FieldRt::io read)
static FieldRt field(const uint32_t *p29, uint32_t pinv, const uint32_t *io) {
    FieldRt f;
    for (int i = 0; i < kN; ++i) f.p[i] = p29[i];
    f.pinv = pinv;
    f.unit = 1;
    f.io = io;
    return f;
}

// words: [n][8] in, canonical integers out (in place)
extern "C" void sc_to_canonical(const uint32_t *p29, uint32_t pinv, const uint32_t *p32, uint32_t *words, size_t n) {
    uint32_t io[kIoWords] = {};
    std::memcpy(io + kIoP32, p32, 32);
    const FieldRt f = field(p29, pinv, io);
    for (size_t i = 0; i < n; ++i) {
        Abi a;
        std::memcpy(a.w, words + i * 8, 32);
        const Abi x = abi_to_canonical(a, f);
        std::memcpy(words + i * 8, x.w, 32);
    }
}

extern "C" uint32_t sc_unit(const uint32_t *p29, int bits) {
    uint32_t io[kIoWords] = {};
    return cut_unit(field(p29, 0, io), bits != 0);
}
extern "C" uint64_t sc_elems(uint64_t len, uint32_t unit) { return cut_elems((size_t)len, unit); }
extern "C" uint64_t sc_offset(uint64_t r, uint32_t e, uint64_t len, uint32_t unit) { return cut_offset(r, e, len, unit); }
extern "C" uint32_t sc_count(uint32_t e, uint64_t len, uint32_t unit) { return cut_count(e, len, unit); }
