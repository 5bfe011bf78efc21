// pmx_merkle_plan.hpp (the host plan of pmx_merkle_ary_update) behind a C interface, for tests/test_merkle_update_plan.py: the test
// replays the device's share - compress the rows of a level, scatter the digests to their slots - with the oracle's hash.
#include <cstdint>

#include "pmx_merkle_plan.hpp"

using pmx::MerkleUpdatePlan;

extern "C" {

void *mp_build(const uint64_t *nodes, size_t n_leaves, uint32_t arity, const uint64_t *indices, const uint64_t *new_leaves, size_t k) {
    MerkleUpdatePlan *p = new MerkleUpdatePlan();
    pmx::merkle_update_plan(nodes, n_leaves, arity, indices, new_leaves, k, p);
    return p;
}
void mp_free(void *h) { delete static_cast<MerkleUpdatePlan *>(h); }
size_t mp_first_bad(const uint64_t *indices, size_t k, size_t n_leaves) { return pmx::merkle_update_first_bad(indices, k, n_leaves); }
size_t mp_depth(void *h) { return static_cast<MerkleUpdatePlan *>(h)->depth; }
size_t mp_n_rows(void *h) { return static_cast<MerkleUpdatePlan *>(h)->n_rows(); }
size_t mp_level_size(void *h, size_t l) { return static_cast<MerkleUpdatePlan *>(h)->level[l].size(); }
const uint64_t *mp_level(void *h, size_t l) { return static_cast<MerkleUpdatePlan *>(h)->level[l].data(); }
size_t mp_level_first(void *h, size_t l) { return static_cast<MerkleUpdatePlan *>(h)->first[l]; }
size_t mp_row_first(void *h, size_t l) { return static_cast<MerkleUpdatePlan *>(h)->row_first[l]; }
size_t mp_upload_words(void *h) { return static_cast<MerkleUpdatePlan *>(h)->upload.size(); }
uint64_t *mp_rows(void *h) { return static_cast<MerkleUpdatePlan *>(h)->rows(); }
const uint64_t *mp_slots(void *h) { return static_cast<MerkleUpdatePlan *>(h)->slots(); }
void mp_apply(void *h, const uint64_t *new_leaves, const uint64_t *digests, uint64_t *nodes) {
    pmx::merkle_update_apply(*static_cast<MerkleUpdatePlan *>(h), new_leaves, digests, nodes);
}

}  // extern "C"
