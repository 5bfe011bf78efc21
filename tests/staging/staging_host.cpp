// pmx_staging.hpp for tests/test_staging.py: the builder behind a C interface.
// Build: g++ -O1 -std=c++17 -fPIC -shared -DPMX_HOSTCHECK -I sponge_amd/csrc tests/staging/staging_host.cpp -o <lib>
#include "pmx_staging.hpp"

extern "C" {
// sections [n] of (count, elem_bytes) added in order: offsets [n] out, *bytes the total; returns the overflow flag
int st_layout(const size_t *count, const size_t *elem_bytes, size_t n, size_t *offsets, size_t *bytes) {
    pmx::Staging s;
    for (size_t i = 0; i < n; ++i) offsets[i] = s.add(count[i], elem_bytes[i]);
    *bytes = s.bytes();
    return s.overflowed() ? 1 : 0;
}
// one section of a * b elements (Staging::times) of elem_bytes bytes behind `lead` bytes
int st_product(size_t lead, size_t a, size_t b, size_t elem_bytes, size_t *offset, size_t *bytes) {
    pmx::Staging s;
    s.add(lead, 1);
    *offset = s.add(s.times(a, b), elem_bytes);
    *bytes = s.bytes();
    return s.overflowed() ? 1 : 0;
}
}
