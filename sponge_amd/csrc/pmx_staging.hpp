// The layout of one device staging block of a host-buffer entry (pmx_ctx.hpp: HostCall::stage), as arithmetic: sections added one behind
// the other, every one on a 16-byte boundary - what the *_dev entries ask of the pointers they are fed.  A size that does not fit size_t
// sets a flag the call scope refuses, so a section's size and its overflow guard are one expression.
// Pure size_t arithmetic, host only: no HIP header, no allocation, in no device translation unit; compiled into tests/staging/ as well.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pmx {

class Staging {
public:
    // a * b, for a section counted in two factors (k rows of row_len elements); the flag is set when the product does not fit
    size_t times(size_t a, size_t b) {
        if (b && a > SIZE_MAX / b) return overflow_ = true, 0;
        return a * b;
    }
    // `count` elements of elem_bytes bytes behind what is there: the section's byte offset.  A section may be empty; the next one then
    // starts where it does.
    size_t add(size_t count, size_t elem_bytes) {
        const size_t size = times(count, elem_bytes);
        if (end_ > SIZE_MAX - 15) return overflow_ = true, 0;
        const size_t at = (end_ + 15) & ~(size_t)15;
        if (size > SIZE_MAX - at) return overflow_ = true, 0;
        end_ = at + size;
        return at;
    }
    size_t bytes() const { return end_; }           // the end of the last section (nothing is padded behind it)
    bool overflowed() const { return overflow_; }   // some product or sum did not fit: offsets and bytes() mean nothing

private:
    size_t end_ = 0;
    bool overflow_ = false;
};

}  // namespace pmx
