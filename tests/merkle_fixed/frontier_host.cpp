// sponge_amd/csrc/pmx_merkle_frontier.hpp under ASan + UBSan, a program of its own (tests/test_merkle_fixed_host.py builds and runs it):
// for k in {2, 3, 8}, every depth D with k^D <= 4096, every n and every m with n + m <= k^D, the plan of an append against the
// definitions restated here by plain division - row counts per level, the partial node's position, pads, frontier digits - and the walk
// replayed on the plan's own lists: a slot is read only after it was placed, and placed once.  The replay runs on intervals for every
// (n, m) and, slot by slot on a map of the whole device array, for every (n, m) of the trees of at most 256 positions.
//   frontier_host                     the sweep; prints "sanitized ok"
//   frontier_host plan n m k D        the levels of one plan, one line each: first kept fresh partial pads parents digit digit_slot offset
#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <thread>
#include <utility>
#include <vector>

#include "pmx_merkle_frontier.hpp"

using namespace pmx;

#define CHECK(cond)                                                                                              \
    do {                                                                                                         \
        if (!(cond)) {                                                                                           \
            std::fprintf(stderr, "%s:%d: %s   (k=%u D=%zu n=%llu m=%llu)\n", __FILE__, __LINE__, #cond, k, D, \
                         (unsigned long long)n, (unsigned long long)m);                                          \
            std::abort();                                                                                        \
        }                                                                                                        \
    } while (0)

// floor(x / pw) for pw = k^l <= 2^64
static uint64_t over(uint64_t x, u128 pw) { return pw >> 64 ? 0 : x / (uint64_t)pw; }

// the plan against the definitions; `slots`: also replay the walk on a map of every element of the device array
static void check_plan(uint64_t n, uint64_t m, uint32_t k, size_t D, bool slots) {
    static thread_local FrontierPlan P;
    CHECK(frontier_plan(n, m, k, D, &P) == FrontierError::ok);
    CHECK(P.level.size() == D + 1 && P.arity == k && P.depth == D && P.n == n && P.m == m);
    const uint64_t total = n + m;
    const size_t fe = D * (k - 1);
    CHECK(P.in_frontier == 0 && P.in_defaults == fe && P.out_frontier == fe + D + 1 && P.out_root == P.out_frontier + fe);
    size_t cursor = P.out_root + 1, place_at = 0, gather_at = 0;
    u128 pw = 1;
    for (size_t l = 0; l <= D; ++l, pw *= k) {
        const FrontierLevel &L = P.level[l];
        const u128 f = over(n, pw), g = over(total, pw);            // complete nodes before and after
        // node j is complete iff (j + 1) k^l <= n: f is their number; the partial node is node g and exists iff g k^l < n + m
        CHECK((f + 1) * pw > n && f * pw <= n && (g + 1) * pw > total && g * pw <= total);
        CHECK(L.fresh == (uint64_t)(g - f));
        CHECK(L.partial == (g * pw < total ? 1u : 0u));
        CHECK(L.offset == cursor);
        if (l == D) {
            CHECK(L.kept == 0 && L.pads == 0 && L.parents == 0 && L.rows() <= 1);
            cursor += 1;
            break;
        }
        CHECK(L.kept == (uint64_t)(f % k) && L.first == (uint64_t)(f / k * k) && L.first + L.kept == (uint64_t)f);
        CHECK(L.digit == (uint64_t)(g % k) && L.first + L.digit_slot == (uint64_t)(g / k * k));
        CHECK(L.parents == (L.rows() + k - 1) / k && L.pads == L.parents * k - L.rows() && L.pads < k);
        // what the launch writes is what the level above expects behind its kept nodes
        CHECK(P.level[l + 1].fresh + P.level[l + 1].partial == L.parents);
        if (l == 0) CHECK(L.fresh == m && L.partial == 0);
        // the row is tiled without a gap: kept (placed), fresh and partial (the leaves, or the launch below), pads (placed)
        for (uint64_t j = 0; j < L.kept; ++j, place_at += 2)
            CHECK(P.place[place_at] == L.offset + j && P.place[place_at + 1] == P.in_frontier + l * (k - 1) + j);
        for (uint64_t j = 0; j < L.pads; ++j, place_at += 2)
            CHECK(P.place[place_at] == L.offset + L.rows() + j && P.place[place_at + 1] == P.in_defaults + l);
        // the new frontier lies inside what the row holds as complete nodes
        CHECK(L.digit_slot + L.digit <= L.kept + L.fresh);
        for (uint64_t j = 0; j < L.digit; ++j, gather_at += 2)
            CHECK(P.gather[gather_at] == P.out_frontier + l * (k - 1) + j && P.gather[gather_at + 1] == L.offset + L.digit_slot + j);
        cursor += (size_t)(L.parents * k);
    }
    CHECK(place_at == P.place.size() && cursor == P.elements);
    CHECK(P.root_computed == (P.level[D].rows() == 1) && P.root_is_default == (total == 0));
    // the root is unknown only for a full tree that nothing is appended to
    CHECK((P.root_computed || P.root_is_default) == !(m == 0 && (u128)n == pw));
    if (P.root_computed) {
        CHECK(P.gather[gather_at] == P.out_root && P.gather[gather_at + 1] == P.level[D].offset);
        gather_at += 2;
    }
    CHECK(gather_at == P.gather.size());
    if (!slots) return;
    std::vector<unsigned char> placed(P.elements, 0);
    auto put = [&](size_t at) {
        CHECK(at < P.elements && !placed[at]);
        placed[at] = 1;
    };
    for (size_t l = 0; l < D; ++l)                                  // the upload: the frontier slots below the digit, every default digest
        for (uint64_t j = 0; j < P.level[l].kept; ++j) put(P.in_frontier + l * (k - 1) + j);
    for (size_t l = 0; l <= D; ++l) put(P.in_defaults + l);
    for (uint64_t j = 0; j < m; ++j) put(P.level[0].offset + P.level[0].kept + j);
    for (size_t i = 0; i < P.place.size(); i += 2) {
        CHECK(P.place[i + 1] < P.out_frontier && placed[P.place[i + 1]]);
        put(P.place[i]);
    }
    for (size_t l = 0; l < D; ++l) {
        const FrontierLevel &L = P.level[l], &U = P.level[l + 1];
        for (uint64_t j = 0; j < L.parents * k; ++j) CHECK(placed[L.offset + j]);
        for (uint64_t j = 0; j < L.parents; ++j) {
            CHECK(U.kept + j < (l + 1 < D ? U.parents * k : 1));      // inside the row above
            put(U.offset + U.kept + j);
        }
    }
    for (size_t i = 0; i < P.gather.size(); i += 2) {
        CHECK(P.gather[i + 1] < P.elements && placed[P.gather[i + 1]]);
        CHECK(P.gather[i] >= P.out_frontier && P.gather[i] <= P.out_root);
        put(P.gather[i]);
    }
}

static void sweep(uint32_t k, size_t D, uint64_t capacity) {
    const unsigned workers = 8;
    std::vector<std::thread> pool;
    for (unsigned w = 0; w < workers; ++w)
        pool.emplace_back([=] {
            for (uint64_t n = w; n <= capacity; n += workers)
                for (uint64_t m = 0; n + m <= capacity; ++m) check_plan(n, m, k, D, capacity <= 256);
        });
    for (auto &t : pool) t.join();
}

int main(int argc, char **argv) {
    if (argc == 6 && std::string_view(argv[1]) == "plan") {
        const uint64_t n = std::strtoull(argv[2], nullptr, 10), m = std::strtoull(argv[3], nullptr, 10);
        const uint32_t k = (uint32_t)std::strtoul(argv[4], nullptr, 10);
        const size_t D = std::strtoul(argv[5], nullptr, 10);
        FrontierPlan P;
        const FrontierError e = frontier_plan(n, m, k, D, &P);
        if (e != FrontierError::ok) {
            std::printf("refused %d\n", (int)e);
            return 0;
        }
        for (const FrontierLevel &L : P.level)
            std::printf("%llu %llu %llu %llu %llu %llu %llu %llu %zu\n", (unsigned long long)L.first, (unsigned long long)L.kept,
                        (unsigned long long)L.fresh, (unsigned long long)L.partial, (unsigned long long)L.pads, (unsigned long long)L.parents,
                        (unsigned long long)L.digit, (unsigned long long)L.digit_slot, L.offset);
        return 0;
    }
    for (uint32_t k : {2u, 3u, 8u}) {
        uint64_t capacity = k;
        for (size_t D = 1; capacity <= 4096; ++D, capacity *= k) sweep(k, D, capacity);
    }
    // k^D = 2^64: every count a size_t can hold fits, the root of such a tree is always a partial node or the default
    {
        const uint32_t k = 2;
        const size_t D = 64;
        u128 capacity = 0;
        uint64_t n = 0, m = 0;
        CHECK(frontier_capacity(2, 64, &capacity) == FrontierError::ok && capacity == (u128)1 << 64);
        const uint64_t top = UINT64_MAX;
        for (auto nm : {std::pair<uint64_t, uint64_t>{0, 0}, {0, 1}, {1, 0}, {top, 0}, {top - 1, 1}, {top - 4096, 4096}, {(uint64_t)1 << 63, 1},
                        {((uint64_t)1 << 63) - 1, 2}, {0x123456789abcdefull, 1000}}) {
            n = nm.first, m = nm.second;
            check_plan(n, m, k, D, false);
            FrontierPlan P;
            CHECK(frontier_plan(n, m, k, D, &P) == FrontierError::ok);
            CHECK(P.level[D].fresh == 0 && P.level[D].partial == (n + m ? 1u : 0u));
        }
        FrontierPlan P;
        n = top, m = 1;                                              // 2^64 leaves do not fit the count
        CHECK(frontier_plan(n, m, k, D, &P) == FrontierError::too_many);
        n = 1, m = top - 1;
        CHECK(frontier_plan(n, m, k, D, &P) == FrontierError::bytes_overflow);
    }
    {
        uint32_t k = 2;
        size_t D = 65;
        uint64_t n = 0, m = 0;
        u128 capacity = 0;
        FrontierPlan P;
        std::vector<size_t> first;
        CHECK(frontier_capacity(2, 65, &capacity) == FrontierError::depth && frontier_plan(0, 1, 2, 65, &P) == FrontierError::depth);
        CHECK(frontier_capacity(3, 41, &capacity) == FrontierError::pow_overflow && frontier_plan(0, 1, 3, 41, &P) == FrontierError::pow_overflow);
        CHECK(fixed_shape(1, 3, 41, &first) == FrontierError::pow_overflow && fixed_shape(1, 2, 65, &first) == FrontierError::depth);
        CHECK(frontier_capacity(3, 40, &capacity) == FrontierError::ok && capacity == (u128)12157665459056928801ull);
        CHECK(frontier_capacity(1, 4, &capacity) == FrontierError::arity && frontier_capacity(2, 0, &capacity) == FrontierError::depth);
        k = 3, D = 40, n = 12157665459056928800ull, m = 1;
        check_plan(n, m, k, D, false);
        CHECK(frontier_plan(n, 2, k, D, &P) == FrontierError::too_many);
        // the dense shape: level l stores max(1, ceil(n / k^l)) nodes
        k = 3, D = 4;
        for (n = 1; n <= 81; ++n) {
            CHECK(fixed_shape(n, k, D, &first) == FrontierError::ok && first.size() == D + 2 && first[0] == 0);
            uint64_t pw = 1;
            for (size_t l = 0; l <= D; ++l, pw *= k) CHECK(first[l + 1] - first[l] == (n + pw - 1) / pw);
        }
        CHECK(fixed_shape(0, k, D, &first) == FrontierError::no_leaves && fixed_shape(82, k, D, &first) == FrontierError::too_many);
        CHECK(fixed_shape((uint64_t)1 << 60, 2, 64, &first) == FrontierError::bytes_overflow);
    }
    std::puts("sanitized ok");
    return 0;
}
