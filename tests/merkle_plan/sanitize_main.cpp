// pmx_merkle_plan.hpp under ASan + UBSan (tests/test_merkle_update_plan.py builds and runs this program on its own): plans over trees
// of arities 2, 3, 8 and 15 and depths 0 .. 4 are replayed the way the device runs them - compress the rows of a level, scatter the
// digests to their slots of the next level's rows - with a stand-in compression, and the result must be the full rebuild with the same
// compression.  The stand-in only has to make every node depend on all of its children and on their order.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pmx_merkle_plan.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static void compress(const uint64_t *row, uint32_t arity, uint64_t *out) {
    uint64_t h[4] = {1, 2, 3, 4};
    for (uint32_t c = 0; c < arity; ++c)
        for (int w = 0; w < 4; ++w) {
            h[w] = (h[w] ^ row[c * 4 + w]) * 0x100000001B3ull + c;
            h[(w + 1) & 3] += h[w] >> 29;
        }
    std::memcpy(out, h, 32);
}

static std::vector<uint64_t> rebuild(const std::vector<uint64_t> &leaves, uint32_t arity) {
    std::vector<uint64_t> nodes = leaves;
    size_t first = 0, width = leaves.size() / 4;
    while (width > 1) {
        nodes.resize((first + width + width / arity) * 4);
        for (size_t p = 0; p < width / arity; ++p) compress(&nodes[(first + p * arity) * 4], arity, &nodes[(first + width + p) * 4]);
        first += width;
        width /= arity;
    }
    return nodes;
}

static int run(uint32_t arity, size_t depth, const std::vector<uint64_t> &indices) {
    size_t n = 1;
    for (size_t l = 0; l < depth; ++l) n *= arity;
    std::vector<uint64_t> leaves(n * 4);
    for (auto &w : leaves) w = rnd();
    std::vector<uint64_t> nodes = rebuild(leaves, arity);
    const size_t k = indices.size();
    std::vector<uint64_t> fresh(k * 4 + 4);
    for (auto &w : fresh) w = rnd();
    for (size_t i = 0; i < k; ++i) std::memcpy(&leaves[indices[i] * 4], &fresh[i * 4], 32);     // in call order: the last one wins
    const std::vector<uint64_t> want = rebuild(leaves, arity);

    if (pmx::merkle_update_first_bad(indices.data(), k, n) != k) return 1;
    pmx::MerkleUpdatePlan plan;
    pmx::merkle_update_plan(nodes.data(), n, arity, indices.data(), fresh.data(), k, &plan);
    if (plan.depth != depth) return 2;
    std::vector<uint64_t> digests(plan.n_rows() * 4 + 4);
    uint64_t *rows = plan.rows();
    const uint64_t *slots = plan.slots();
    for (size_t l = 1; l <= depth; ++l) {
        const size_t r = plan.row_first[l], count = plan.level_rows(l);
        for (size_t j = 0; j < count; ++j) compress(rows + (r + j) * arity * 4, arity, &digests[(r + j) * 4]);
        if (l < depth)
            for (size_t j = 0; j < count; ++j) {
                if (slots[r + j] >= plan.level_rows(l + 1) * arity) return 3;
                std::memcpy(rows + (plan.row_first[l + 1] * arity + slots[r + j]) * 4, &digests[(r + j) * 4], 32);
            }
    }
    pmx::merkle_update_apply(plan, fresh.data(), digests.data(), nodes.data());
    return nodes == want ? 0 : 4;
}

int main() {
    int cases = 0;
    for (uint32_t arity : {2u, 3u, 8u, 15u})
        for (size_t depth = 0; depth <= 4; ++depth) {
            size_t n = 1;
            for (size_t l = 0; l < depth; ++l) n *= arity;
            std::vector<std::vector<uint64_t>> sets;
            sets.push_back({});
            sets.push_back({0});
            sets.push_back({n - 1});
            sets.push_back({0, n - 1, 0, n - 1, 0});                            // duplicates
            std::vector<uint64_t> one_parent, all, random;
            for (size_t c = 0; c < arity && c < n; ++c) one_parent.push_back(n - 1 - c);
            for (size_t i = 0; i < n && i < 4096; ++i) all.push_back(n - 1 - i);
            for (size_t i = 0; i < 97; ++i) random.push_back(rnd() % n);
            sets.push_back(one_parent);
            sets.push_back(all);
            sets.push_back(random);
            for (const auto &s : sets) {
                const int rc = run(arity, depth, s);
                if (rc) {
                    std::printf("arity %u depth %zu k %zu: failure %d\n", arity, depth, s.size(), rc);
                    return 1;
                }
                ++cases;
            }
        }
    const uint64_t bad[3] = {5, 81, 7};
    if (pmx::merkle_update_first_bad(bad, 3, 81) != 1 || pmx::merkle_update_first_bad(bad, 1, 81) != 1) return 1;
    std::printf("sanitized ok: %d plans\n", cases);
    return 0;
}
