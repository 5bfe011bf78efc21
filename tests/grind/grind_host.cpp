// The host-compilable pieces of the grinding search (pmx_sponge_grind), a program of its own under ASan + UBSan (tests/test_grind_host.py
// builds and runs it; nothing sanitized is loaded into the test process):
//   abi_from_u64 (pmx_field.hpp)    integer -> ABI residue v * 2^256 mod p, what grind_kernel absorbs per candidate, with the constant
//                                   2^517 mod p laid out as pmx_prepare.hpp lays it out behind FieldRt::io
//   canonical_low_bits_zero         the acceptance test on the canonical digest
//   pmx_grind_plan.hpp              the chunk walk of the host loop
// usage: grind_host                      self-checks against pmx_host_field.hpp (the code behind pmx_to_mont), prints "sanitized ok"
//        grind_host residues             "<modulus name> <v> <residue as 64 hex digits>" for the corner integers on both product fields
//        grind_host walk <first> <count> <chunk>      "<first> <count>" of every chunk, in the order the host loop launches them
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "pmx_field.hpp"
#include "pmx_grind_plan.hpp"
#include "pmx_host_field.hpp"

namespace pmx {
void hostcheck_track(int, const Fe &, const FieldRt &) {}
void hostcheck_below_2_256(const Fe &) {}
}  // namespace pmx

using namespace pmx;

static const uint64_t kBls[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
static const uint64_t kBn254[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
static const uint64_t kCorners[6] = {0, 1, 0xffffffffull, 0x100000000ull, 0x8000000000000000ull, 0xffffffffffffffffull};

static void limbs29(const U256 &v, uint32_t *out) {
    for (int i = 0; i < kN; ++i) {
        const int bit = kW * i, w = bit / 64, sh = bit % 64;
        uint64_t x = v.l[w] >> sh;
        if (sh + kW > 64 && w + 1 < 4) x |= v.l[w + 1] << (64 - sh);
        out[i] = (uint32_t)x & kMask;
    }
}

struct HostRt {
    HostField hf;
    uint32_t io[kIoWords];
    FieldRt f;
    explicit HostRt(const uint64_t modulus[4]) {
        if (!hf.init(modulus)) std::abort();
        std::memset(io, 0, sizeof io);
        std::memcpy(io + kIoP32, hf.p.l, 32);
        U256 c = hf.r2;   // 2^512 mod p -> 2^517 mod p
        for (int i = 0; i < 5; ++i) c = hf.add(c, c);
        limbs29(c, io + kIoFromU64);
        limbs29(hf.p, f.p);
        f.pinv = (uint32_t)hf.inv & kMask;
        f.unit = 1;
        f.io = io;
    }
    U256 residue(uint64_t v) const {
        const Abi a = abi_from_u64(v, f);
        U256 r;
        std::memcpy(r.l, a.w, 32);
        return r;
    }
};

static int fail(const char *what) {
    std::printf("FAILED: %s\n", what);
    return 1;
}

static int self_check() {
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (const uint64_t *modulus : {kBls, kBn254}) {
        const HostRt rt(modulus);
        for (int i = 0; i < 6 + 2000; ++i) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            const uint64_t v = i < 6 ? kCorners[i] : x >> (i % 64);
            const U256 got = rt.residue(v), want = rt.hf.to_mont(U256{{v, 0, 0, 0}});
            if (std::memcmp(got.l, want.l, 32)) return fail("abi_from_u64 differs from to_mont");
        }
    }
    // the acceptance test against a bit loop
    for (int i = 0; i < 4000; ++i) {
        Abi a;
        for (int w = 0; w < 8; ++w) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            a.w[w] = (i & 1) ? 0u : (uint32_t)x;
        }
        const uint32_t low = (uint32_t)(x % 257);            // zero bits at the bottom
        for (uint32_t b = 0; b < low; ++b) a.w[b / 32] &= ~(1u << (b % 32));
        if (low < 256) a.w[low / 32] |= 1u << (low % 32);   // ... and exactly that many
        for (uint32_t bits = 0; bits <= 256; ++bits)
            if (canonical_low_bits_zero(a, bits) != (bits <= low)) return fail("canonical_low_bits_zero");
    }
    // the walk: ascending, disjoint, exactly the range - count below one chunk, one chunk, a short last chunk, ranges that end at 2^64
    struct Case { uint64_t first, count, chunk; };
    const Case cases[] = {{0, 1, 1 << 20}, {5, 300, 1 << 20}, {0, 1 << 20, 1 << 20}, {7, (1 << 20) + 1, 1 << 20}, {0, 1000, 64}, {3, 1001, 64},
                          {UINT64_MAX - 299, 300, 64}, {UINT64_MAX - 299, 300, 1 << 20}, {UINT64_MAX, 1, 1}, {0, UINT64_MAX, UINT64_MAX / 3},
                          {1, UINT64_MAX, (uint64_t)1 << 62}, {(uint64_t)1 << 32, 5000, 4096}};
    for (const Case &c : cases) {
        if (!grind_range_ok(c.first, c.count)) return fail("grind_range_ok refuses a valid range");
        const uint64_t chunks = grind_chunks(c.count, c.chunk);
        uint64_t next = c.first, total = 0;
        for (uint64_t k = 0; k < chunks; ++k) {
            const GrindChunk g = grind_chunk_at(c.first, c.count, c.chunk, k);
            if (g.first != next || g.count == 0 || g.count > c.chunk) return fail("chunk out of order or out of size");
            if (g.count - 1 > UINT64_MAX - g.first) return fail("chunk leaves the 64-bit nonces");
            if (k + 1 < chunks && g.count != c.chunk) return fail("a chunk before the last is short");
            next = g.first + g.count;   // (wraps to 0 behind a range that ends at 2^64: only then, and only behind the last chunk)
            total += g.count;
        }
        if (total != c.count || next != c.first + c.count) return fail("the chunks do not cover the range");
    }
    if (grind_chunks(0, 64) != 0 || !grind_range_ok(UINT64_MAX, 0) || !grind_range_ok(0, UINT64_MAX) || !grind_range_ok(1, UINT64_MAX))
        return fail("empty / full ranges");
    if (grind_range_ok(2, UINT64_MAX) || grind_range_ok(UINT64_MAX, 2) || grind_range_ok(UINT64_MAX - 299, 301)) return fail("an overflowing range passes");
    std::printf("sanitized ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 1) return self_check();
    if (!std::strcmp(argv[1], "residues")) {
        int m = 0;
        for (const uint64_t *modulus : {kBls, kBn254}) {
            const HostRt rt(modulus);
            for (uint64_t v : kCorners) {
                const U256 r = rt.residue(v);
                std::printf("%s %" PRIu64 " %016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "\n", m ? "bn254_fr" : "bls12_381_fr", v, r.l[3], r.l[2],
                            r.l[1], r.l[0]);
            }
            ++m;
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "walk") && argc == 5) {
        const uint64_t first = std::strtoull(argv[2], nullptr, 10), count = std::strtoull(argv[3], nullptr, 10), chunk = std::strtoull(argv[4], nullptr, 10);
        if (!grind_range_ok(first, count) || chunk == 0) {
            std::printf("refused\n");
            return 0;
        }
        const uint64_t chunks = grind_chunks(count, chunk);
        for (uint64_t k = 0; k < chunks; ++k) {
            const GrindChunk g = grind_chunk_at(first, count, chunk, k);
            std::printf("%" PRIu64 " %" PRIu64 "\n", g.first, g.count);
        }
        return 0;
    }
    return 2;
}
