// squeeze_bytes / squeeze_bits of a batch (src/poseidon/mod.rs:256-286) as arithmetic on positions: how many native elements a row of
// `len` output units needs, where element e of row r lands in the packed output and how many units it contributes.  A unit is a byte
// of squeeze_bytes or a bit of squeeze_bits (stored as one byte holding 0 or 1); `unit` is what one element yields:
//     bytes: (MODULUS_BIT_SIZE - 1) / 8      (mod.rs:257  usable_bytes)        28 .. 31 for the moduli this library takes
//     bits :  MODULUS_BIT_SIZE - 1           (mod.rs:274  usable_bits)        224 .. 254
// The rows are packed, so consecutive elements (row-major) write consecutive output: cut_offset is monotone in r * elems + e and
// cut_offset(r, e) + cut_count(e) is the offset of the next element, also across a row's truncated last element.
// Host and device (the conversion kernels of pmx_convert.hip, the API's size checks, tests/squeeze_cut/).
#pragma once
#include <cstddef>
#include <cstdint>

#include "pmx_field.hpp"

namespace pmx {

// bit length of the modulus held as 9 x 29-bit limbs
PMX_FN uint32_t modulus_bits(const FieldRt &f) {
    for (int i = kN - 1; i >= 0; --i)
        if (f.p[i]) return (uint32_t)(i * kW + 32 - __builtin_clz(f.p[i]));
    return 0;
}
PMX_FN uint32_t cut_unit(const FieldRt &f, bool bits) { return bits ? modulus_bits(f) - 1 : (modulus_bits(f) - 1) / 8; }
// native elements one row squeezes: ceil(len / unit)   (mod.rs:258, 275)
PMX_FN size_t cut_elems(size_t len, uint32_t unit) { return len / unit + (len % unit != 0); }
// first output unit of element e of row r
PMX_FN uint64_t cut_offset(uint64_t r, uint32_t e, uint64_t len, uint32_t unit) { return r * len + (uint64_t)e * unit; }
// units element e contributes: `unit`, or what is left of the row (the truncation of mod.rs:268, 284); e < cut_elems(len, unit)
PMX_FN uint32_t cut_count(uint32_t e, uint64_t len, uint32_t unit) {
    const uint64_t left = len - (uint64_t)e * unit;
    return left < unit ? (uint32_t)left : unit;
}

}  // namespace pmx
