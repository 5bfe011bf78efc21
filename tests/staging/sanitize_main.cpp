// pmx_staging.hpp under ASan + UBSan (tests/test_staging.py builds and runs this program on its own; nothing sanitized is loaded into
// the test process).  The ranges of the Python test: every pair of sections of 0 .. 40 elements of 1, 4, 8 and 32 bytes walks a buffer of
// exactly bytes() bytes, section by section; the products and sums around SIZE_MAX set the flag without a signed or wrapped step.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pmx_staging.hpp"

using namespace pmx;

static int fail(const char *what, size_t a, size_t b, size_t c) {
    std::printf("FAILED: %s (%zu, %zu, %zu)\n", what, a, b, c);
    return 1;
}

int main() {
    size_t layouts = 0, edges = 0;
    for (size_t e1 : {1, 4, 8, 32})
        for (size_t e2 : {1, 4, 8, 32})
            for (size_t n1 = 0; n1 <= 40; ++n1)
                for (size_t n2 = 0; n2 <= 40; ++n2) {
                    Staging s;
                    const size_t a = s.add(n1, e1), b = s.add(n2, e2), c = s.add(3, 8);
                    if (s.overflowed()) return fail("a small layout overflows", n1, n2, e1);
                    if (a != 0 || b != (n1 * e1 + 15) / 16 * 16 || c != (b + n2 * e2 + 15) / 16 * 16) return fail("offsets", n1, n2, e1);
                    if (s.bytes() != c + 24) return fail("bytes", n1, n2, e1);
                    std::vector<unsigned char> block(s.bytes(), 0);     // every section written inside a block of exactly bytes()
                    for (size_t i = 0; i < n1 * e1; ++i) block[a + i] += 1;
                    for (size_t i = 0; i < n2 * e2; ++i) block[b + i] += 1;
                    for (size_t i = 0; i < 24; ++i) block[c + i] += 1;
                    for (unsigned char x : block)
                        if (x > 1) return fail("sections overlap", n1, n2, e1);
                    ++layouts;
                }
    for (size_t elem : {3, 8, 32, 96}) {     // (at 1 byte there is no count beyond SIZE_MAX)
        Staging fits, over, padded;
        fits.add(SIZE_MAX / elem, elem);
        if (fits.overflowed() || fits.bytes() != SIZE_MAX / elem * elem) return fail("SIZE_MAX / elem must fit", elem, 0, 0);
        over.add(SIZE_MAX / elem + 1, elem);
        if (!over.overflowed()) return fail("SIZE_MAX / elem + 1 must not fit", elem, 0, 0);
        padded.add(16, 1);
        padded.add(SIZE_MAX - 31, 1);    // ends at SIZE_MAX - 15, a boundary
        padded.add(1, 1);                // ends at SIZE_MAX - 14
        if (padded.overflowed()) return fail("the plain sum fits", elem, 1, 0);
        padded.add(14, 1);               // 16 + (SIZE_MAX - 31) + 1 + 14 = SIZE_MAX fits; its aligned start does not
        if (!padded.overflowed()) return fail("the padding must overflow", elem, 2, 0);
        Staging product;
        if (product.times(SIZE_MAX / elem, elem) != SIZE_MAX / elem * elem || product.overflowed()) return fail("times fits", elem, 3, 0);
        (void)product.times(SIZE_MAX / elem + 1, elem);
        if (!product.overflowed()) return fail("times must not fit", elem, 4, 0);
        ++edges;
    }
    std::printf("sanitized ok: %zu layouts, %zu edges\n", layouts, edges);
    return 0;
}
