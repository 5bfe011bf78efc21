// How the host-buffer sponge entries (pmx_sponge.cpp: resident_walk behind sponge_host and squeeze_cut_host; varlen_host) cut a call that is longer than one device
// call may be.  The pass drivers launch one kernel per permutation a sponge of the call can need, and a device call is limited to
// kMaxPasses of them: kMaxPasses rates of elements per sponge.  The reference takes any length (src/poseidon/mod.rs:232-254, 321-341),
// so the host entries walk a longer call in pieces, the sponges resident on the device in between.
// Pure size_t arithmetic, host only: no HIP header, in no device translation unit; compiled into tests/host_pieces/ as well.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pmx {

// launches = permutations a sponge of one device call can need.  The limit is the same for EVERY absorb and squeeze call, whichever
// engine the width and the batch size select (the per-lane kernels loop inside one launch and would not need it: a caller's length
// limit must not depend on its batch size).
constexpr size_t kMaxPasses = 65536;
// fixed_piece shortens a piece of kMaxPasses rates by one rate: what is left must not itself be one rate (nor nothing)
static_assert(kMaxPasses >= 3, "the shortened piece, max_len - rate, must not itself be exactly one rate");

// The next piece of a call of `total` elements per sponge of which `done` < total are behind it (total = 0: the one empty piece);
// max_len is the most one device call takes, a multiple of `rate` and at least three rates (the entries pass kMaxPasses * rate).
// To a duplex sponge absorb(a ++ b) is absorb(a); absorb(b), and squeeze(k1 + k2) is squeeze(k1); squeeze(k2) UNLESS the second call
// asks for exactly `rate` elements from a sponge that stands inside its rate: the test of mod.rs:175 then skips a permutation the long
// call performs.  So the piece is min(total - done, max_len), one rate shorter when exactly one rate would be left behind it: no piece
// but the first - which is the caller's own call when it is the only one - is exactly one rate.
inline size_t fixed_piece(size_t done, size_t total, size_t max_len, size_t rate) {
    const size_t left = total - done, piece = left < max_len ? left : max_len;
    return left - piece == rate ? piece - rate : piece;
}

// The ragged cut of an absorb whose longest row has `longest` elements: piece k takes elements [k * piece, (k + 1) * piece) of every
// row - nothing of a row that ends before it, and the empty piece of such a row changes nothing (mod.rs:234-236).  Absorbing needs no
// one-rate rule.
inline size_t ragged_pieces(size_t longest, size_t piece) { return longest / piece + (longest % piece != 0); }
struct RowRange {
    size_t lo, hi;   // elements [lo, hi) of the row, lo <= hi <= its length
};
inline RowRange ragged_range(size_t len, size_t piece, size_t k) {
    const size_t a = k * piece, b = a + piece;
    return RowRange{len < a ? len : a, len < b ? len : b};
}
// off [n + 1]: the offsets of piece k packed row after row from 0 - with one piece, the caller's offsets minus offsets[0]
// (offsets [n + 1], non-decreasing)
inline void ragged_offsets(const uint64_t *offsets, size_t n, size_t piece, size_t k, uint64_t *off) {
    off[0] = 0;
    for (size_t i = 0; i < n; ++i) {
        const RowRange r = ragged_range((size_t)(offsets[i + 1] - offsets[i]), piece, k);
        off[i + 1] = off[i] + (r.hi - r.lo);
    }
}

}  // namespace pmx
