// pmx_merkle_shape.hpp under ASan + UBSan (tests/test_merkle_shape.py builds and runs this program on its own): every leaf count
// 1 .. 2000 at every arity 2 .. 16 against a walk written out here, and the edges where a size stops fitting - the largest power of
// each arity in a size_t, SIZE_MAX / 32 leaves and one more, both forest bounds, arity^depth at the last depth that fits 64 bits.
// UBSan traps any signed overflow, shift or division by zero on the way; the unsigned arithmetic is checked against 128-bit sums.
#include <cstdint>
#include <cstdio>

#include "pmx_merkle_shape.hpp"

using namespace pmx;
using E = MerkleShapeError;
typedef unsigned __int128 u128;

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("line %d: %s\n", __LINE__, #cond);           \
            ++failures;                                              \
        }                                                            \
    } while (0)

// depth and node count with 128-bit sums; false if n is no power of the arity (exact only)
static bool model(u128 n, uint32_t a, bool exact, size_t *depth, u128 *nodes) {
    *depth = 0, *nodes = 0;
    for (;; n = (n + a - 1) / a, ++*depth) {
        *nodes += n;
        if (n == 1) return true;
        if (exact && n % a) return false;
    }
}

static void small_counts() {
    for (uint32_t a = 2; a <= 16; ++a)
        for (size_t n = 1; n <= 2000; ++n) {
            size_t depth;
            u128 nodes;
            const bool power = model(n, a, true, &depth, &nodes);
            MerkleShape s{77, 77};
            CHECK(merkle_shape(n, a, true, &s) == (power ? E::ok : E::not_power));
            CHECK(power ? (s.depth == depth && s.n_nodes == (size_t)nodes) : (s.depth == 77 && s.n_nodes == 77));
            model(n, a, false, &depth, &nodes);
            CHECK(merkle_shape(n, a, false, &s) == E::ok && s.depth == depth && s.n_nodes == (size_t)nodes);
            // the cursor: level l + 1 follows level l, ceil(width / arity) wide; the switch level of an update
            MerkleLevel lv{0, n, a};
            for (size_t l = 0; l < depth; ++l) {
                const size_t parents = (lv.width + a - 1) / a;
                CHECK(lv.parents() == parents);
                const size_t ks[] = {1, 2, parents - 1, parents, parents + 1};
                for (size_t k : ks) {
                    if (k == 0) continue;
                    const size_t sw = merkle_update_switch_level(n, a, k);
                    CHECK(k >= parents ? sw <= l : sw > l);
                }
                const size_t end = lv.first + lv.width;
                lv.advance();
                CHECK(lv.first == end && lv.width == parents);
            }
            CHECK(lv.width == 1 && lv.first + 1 == s.n_nodes);
            CHECK(merkle_update_switch_level(n, a, n) == 0);
        }
}

static void edges() {
    MerkleShape s;
    size_t tl = 0, tn = 0, depth;
    u128 nodes;
    CHECK(merkle_shape(8, 0, false, &s) == E::arity && merkle_shape(8, 1, true, &s) == E::arity);
    CHECK(merkle_shape(0, 2, false, &s) == E::no_leaves && merkle_shape(0, 2, true, &s) == E::no_leaves);
    for (uint32_t a = 2; a <= 16; ++a) {
        // the powers of the arity: accepted while the node array's bytes fit, the largest in a size_t does not
        size_t n = 1;
        for (;; n *= a) {
            model(n, a, true, &depth, &nodes);
            const bool fits = nodes * 32 <= (u128)SIZE_MAX;
            CHECK(merkle_shape(n, a, true, &s) == (fits ? E::ok : E::tree_overflow));
            CHECK(merkle_shape(n, a, false, &s) == (fits ? E::ok : E::tree_overflow));
            if (fits) CHECK(s.depth == depth && s.n_nodes == (size_t)nodes);
            if (n > SIZE_MAX / a) break;
        }
        model(n, a, true, &depth, &nodes);
        CHECK(nodes * 32 > (u128)SIZE_MAX);
        // arity^depth in 64 bits: `depth` is the last one that fits
        uint64_t got = 0;
        CHECK(merkle_leaves_of_depth(a, depth, &got) == E::ok && got == n);
        CHECK(merkle_leaves_of_depth(a, depth + 1, &got) == E::pow_overflow && got == n);
        CHECK(merkle_leaves_of_depth(a, 0, &got) == E::ok && got == 1);
        // any count: SIZE_MAX / 32 leaves cannot fit with their parents, and the largest count that fits is found by bisection
        CHECK(merkle_shape(SIZE_MAX / 32, a, false, &s) == E::tree_overflow && merkle_shape(SIZE_MAX / 32 + 1, a, false, &s) == E::tree_overflow);
        size_t lo = 1, hi = SIZE_MAX / 32;
        while (lo < hi) {
            const size_t mid = lo + (hi - lo + 1) / 2;
            model(mid, a, false, &depth, &nodes);
            if (nodes <= (u128)(SIZE_MAX / 32)) lo = mid;
            else hi = mid - 1;
        }
        CHECK(merkle_shape(lo, a, false, &s) == E::ok && merkle_shape(lo + 1, a, false, &s) == E::tree_overflow);
        // forests: both bounds, on both sides
        const size_t lpt = (size_t)a * a * a;
        model(lpt, a, true, &depth, &nodes);
        const size_t by_nodes = (SIZE_MAX / 32) / (size_t)nodes, by_pairs = (SIZE_MAX / 128) / lpt;
        CHECK(merkle_forest_shape(by_nodes, lpt, a, false, &tl, &tn) == E::ok && tl == by_nodes * lpt && tn == by_nodes * (size_t)nodes);
        CHECK(merkle_forest_shape(by_nodes + 1, lpt, a, false, &tl, &tn) == E::forest_overflow && tl == by_nodes * lpt);
        CHECK(merkle_forest_shape(by_pairs, lpt, a, true, &tl, &tn) == E::ok && tl == by_pairs * lpt && tn == by_pairs * (size_t)nodes);
        CHECK(merkle_forest_shape(by_pairs + 1, lpt, a, true, &tl, &tn) == E::forest_overflow);
        CHECK(merkle_forest_shape(0, lpt, a, false, &tl, &tn) == E::no_trees && merkle_forest_shape(3, lpt + 1, a, false, &tl, &tn) == E::not_power);
        CHECK(merkle_forest_shape(0, 0, a, true, &tl, &tn) == E::no_leaves && merkle_forest_shape(1, 1, a, true, &tl, &tn) == E::ok && tl == 1 && tn == 1);
    }
    uint64_t got = 5;
    CHECK(merkle_leaves_of_depth(1, 3, &got) == E::arity && got == 5);
    CHECK(merkle_leaves_of_depth(2, 63, &got) == E::ok && got == (uint64_t)1 << 63 && merkle_leaves_of_depth(2, 64, &got) == E::pow_overflow);
    CHECK(merkle_leaves_of_depth(0xffffffffu, 2, &got) == E::ok && got == 0xfffffffe00000001ull && merkle_leaves_of_depth(0xffffffffu, 3, &got) == E::pow_overflow);
}

int main() {
    small_counts();
    edges();
    if (failures) return 1;
    std::printf("sanitized ok: shapes of 2000 leaf counts at 15 arities and the overflow edges\n");
    return 0;
}
