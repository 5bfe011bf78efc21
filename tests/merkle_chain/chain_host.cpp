// The host plan of pmx_merkle_update_witnesses (sponge_amd/csrc/pmx_merkle_chain.hpp) as a program of its own, built by
// tests/test_merkle_chain_host.py with g++ under ASan + UBSan; nothing of it is loaded into the test process.
//
//   chain_host                          the self-check: the source every (level, update, slot) takes when it is chosen from pred alone
//                                       against the overlay model walked literally, on index sets with heavy collisions, all-equal
//                                       indices, k = 1, the ends of a 2^64 tree; prints "sanitized ok"
//   chain_host plan ARITY DEPTH I...    prints pred: per level one line of k * (ARITY - 1) numbers, -1 for none
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string_view>
#include <tuple>
#include <utility>
#include <vector>

#include "pmx_merkle_chain.hpp"

using pmx::ChainPlanner;
using pmx::kChainNone;

namespace {

// (level, slot, who wrote it): who = -1 for the caller's old opening
using Source = std::tuple<size_t, size_t, long long>;

// the overlay model, one update at a time: the writer of every (level, node)
std::vector<Source> literal(const std::vector<uint64_t> &idx, uint32_t a, size_t depth) {
    std::map<std::pair<size_t, uint64_t>, long long> writer;
    std::vector<Source> out;
    for (size_t j = 0; j < idx.size(); ++j) {
        uint64_t q = idx[j];
        for (size_t l = 0; l < depth; ++l, q /= a) {
            const uint64_t digit = q % a, base = q - digit;
            for (size_t s = 0; s + 1 < a; ++s) {
                const auto it = writer.find({l, base + (s < digit ? s : s + 1)});
                out.emplace_back(l, s, it == writer.end() ? -1 : it->second);
            }
        }
        q = idx[j];
        for (size_t l = 0; l <= depth; ++l, q /= a) writer[{l, q}] = (long long)j;
    }
    return out;
}

// the same list chosen from pred alone, the way chain_rows_kernel chooses: an earlier update, or the old opening
std::vector<Source> replayed(const std::vector<uint64_t> &idx, uint32_t a, size_t depth, std::vector<uint32_t> *all_pred) {
    const size_t k = idx.size(), sib = a - 1;
    std::vector<uint32_t> pred(depth * k * sib, 12345u);
    ChainPlanner planner(idx.data(), k, a);
    for (size_t l = 0; l < depth; ++l) planner.next_level(pred.data() + l * k * sib);
    std::vector<Source> out;
    for (size_t j = 0; j < k; ++j)
        for (size_t l = 0; l < depth; ++l)
            for (size_t s = 0; s < sib; ++s) {
                const uint32_t p = pred[(l * k + j) * sib + s];
                if (p != kChainNone && p >= j) {
                    std::printf("pred[%zu][%zu][%zu] = %u is no earlier update\n", l, j, s, p);
                    std::exit(1);
                }
                out.emplace_back(l, s, p < j ? (long long)p : -1);
            }
    if (all_pred) *all_pred = pred;
    return out;
}

size_t checked = 0;
void check(const std::vector<uint64_t> &idx, uint32_t a, size_t depth, const char *what) {
    if (literal(idx, a, depth) != replayed(idx, a, depth, nullptr)) {
        std::printf("FAILED: %s (arity %u, depth %zu, k = %zu)\n", what, a, depth, idx.size());
        std::exit(1);
    }
    ++checked;
}

uint64_t capacity_minus_one(uint32_t a, size_t depth) {
    unsigned __int128 c = 1;
    for (size_t l = 0; l < depth; ++l) c *= a;
    return (uint64_t)(c - 1);
}

int self_check() {
    std::mt19937_64 rng(0xC4A1);
    const std::pair<uint32_t, size_t> shapes[] = {{2, 1}, {2, 4}, {2, 32}, {2, 64}, {3, 3}, {3, 40}, {4, 3}, {8, 2}, {8, 21}, {15, 2}};
    for (const auto &[a, depth] : shapes) {
        const uint64_t top = capacity_minus_one(a, depth);
        check({}, a, depth, "no update");
        for (uint64_t one : {(uint64_t)0, top, top / 2}) check({one}, a, depth, "k = 1");
        for (size_t k : {2, 3, 65, 200}) {
            check(std::vector<uint64_t>(k, top / 3), a, depth, "all equal");
            // heavy collisions: a range of a few leaves; one parent; neighbours at the top end; anywhere in the tree
            for (uint64_t range : {(uint64_t)2, (uint64_t)a, (uint64_t)a * a + 1, (uint64_t)40}) {
                std::vector<uint64_t> low(k), high(k);
                for (size_t j = 0; j < k; ++j) {
                    const uint64_t r = rng() % range;
                    low[j] = r <= top ? r : top;
                    high[j] = top - (r <= top ? r : top);
                }
                check(low, a, depth, "collisions at the low end");
                check(high, a, depth, "collisions at the high end");
            }
            std::vector<uint64_t> wide(k);
            for (size_t j = 0; j < k; ++j) wide[j] = top == UINT64_MAX ? rng() : rng() % (top + 1);
            for (size_t j = 3; j < k; j += 3) wide[j] = wide[j - 3] ^ 1;     // neighbours of earlier updates
            for (uint64_t &x : wide)
                if (x > top) x = top;
            check(wide, a, depth, "anywhere, with neighbours");
        }
    }
    check({0, (uint64_t)1 << 63, UINT64_MAX, 0, UINT64_MAX - 1, ((uint64_t)1 << 63) + 1}, 2, 64, "the ends and the halves of a 2^64 tree");
    // the first index that names no leaf
    const uint64_t some[] = {5, 80, 81, 7};
    if (pmx::chain_first_bad(some, 4, 81, false) != 2 || pmx::chain_first_bad(some, 4, 82, false) != 4 || pmx::chain_first_bad(some, 4, 0, true) != 4 ||
        pmx::chain_first_bad(some, 0, 1, false) != 0) {
        std::printf("FAILED: chain_first_bad\n");
        return 1;
    }
    std::printf("%zu index sets\nsanitized ok\n", checked);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 1) return self_check();
    if (argc < 4 || std::string_view(argv[1]) != "plan") return 2;
    const uint32_t a = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    const size_t depth = std::strtoul(argv[3], nullptr, 10);
    std::vector<uint64_t> idx;
    for (int i = 4; i < argc; ++i) idx.push_back(std::strtoull(argv[i], nullptr, 10));
    std::vector<uint32_t> pred;
    replayed(idx, a, depth, &pred);
    const size_t per = idx.size() * (a - 1);
    for (size_t l = 0; l < depth; ++l) {
        for (size_t i = 0; i < per; ++i) std::printf("%s%lld", i ? " " : "", pred[l * per + i] == kChainNone ? -1LL : (long long)pred[l * per + i]);
        std::printf("\n");
    }
    return 0;
}
