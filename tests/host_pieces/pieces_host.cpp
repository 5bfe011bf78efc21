// pmx_host_pieces.hpp for tests/test_host_pieces.py: the header's functions behind a C interface.
// Build: g++ -O1 -std=c++17 -fPIC -shared -DPMX_HOSTCHECK -I sponge_amd/csrc tests/host_pieces/pieces_host.cpp -o <lib>
#include "pmx_host_pieces.hpp"

extern "C" {
size_t hp_max_passes() { return pmx::kMaxPasses; }
size_t hp_fixed_piece(size_t done, size_t total, size_t max_len, size_t rate) { return pmx::fixed_piece(done, total, max_len, rate); }
size_t hp_ragged_pieces(size_t longest, size_t piece) { return pmx::ragged_pieces(longest, piece); }
void hp_ragged_range(size_t len, size_t piece, size_t k, size_t *lo, size_t *hi) {
    const pmx::RowRange r = pmx::ragged_range(len, piece, k);
    *lo = r.lo;
    *hi = r.hi;
}
void hp_ragged_offsets(const uint64_t *offsets, size_t n, size_t piece, size_t k, uint64_t *off) { pmx::ragged_offsets(offsets, n, piece, k, off); }
}
