// The host walk of a proof-of-work search (pmx_sponge_grind, pmx_sponge.cpp): the nonce range [first, first + count) is searched in
// chunks of at most `chunk` candidates, one launch each, in ascending order, and the walk stops behind the first chunk that reports a
// hit - every nonce of an earlier chunk is smaller than every nonce of a later one, so that chunk's minimum is the range's.
// Pure 64-bit arithmetic, host only; compiled into tests/grind/grind_host.cpp as well.
#pragma once
#include <cstdint>

namespace pmx {

// first + count <= 2^64: the range names nonces that exist (count = 0 is the empty range anywhere)
inline bool grind_range_ok(uint64_t first, uint64_t count) { return count == 0 || count - 1 <= UINT64_MAX - first; }

// launches the whole range takes: ceil(count / chunk), chunk >= 1
inline uint64_t grind_chunks(uint64_t count, uint64_t chunk) { return count / chunk + (count % chunk != 0); }

struct GrindChunk {
    uint64_t first, count;   // nonces first .. first + count - 1; count >= 1 (first + count may be 2^64: never formed)
};
// chunk k < grind_chunks(count, chunk) of a range that passed grind_range_ok: ascending, disjoint, together exactly the range
inline GrindChunk grind_chunk_at(uint64_t first, uint64_t count, uint64_t chunk, uint64_t k) {
    const uint64_t done = k * chunk;   // < count
    return GrindChunk{first + done, count - done < chunk ? count - done : chunk};
}

}  // namespace pmx
