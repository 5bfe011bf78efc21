// pmx_host_pieces.hpp under ASan + UBSan (tests/test_host_pieces.py builds and runs this program on its own; nothing sanitized is
// loaded into the test process).  The ranges of the Python test: the cut of a fixed-length call at rates 1, 2, 3 and 8, max_len of 3, 4
// and 7 rates, every total up to 3 max_len + 2 rates; the ragged cut at pieces of 1, 2 and 5 elements, every longest row up to
// 4 pieces + 2, rows of every length up to the longest in buffers of exactly the size the host entry gives them.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pmx_host_pieces.hpp"

using namespace pmx;

static int fail(const char *what, size_t a, size_t b, size_t c) {
    std::printf("FAILED: %s (%zu, %zu, %zu)\n", what, a, b, c);
    return 1;
}

int main() {
    size_t cuts = 0, raggeds = 0;
    for (size_t rate : {1, 2, 3, 8})
        for (size_t k : {3, 4, 7}) {
            const size_t max_len = k * rate;
            for (size_t total = 0; total <= 3 * max_len + 2 * rate; ++total) {
                size_t done = 0, count = 0;
                do {
                    const size_t piece = fixed_piece(done, total, max_len, rate);
                    if (piece > max_len || piece > total - done) return fail("piece too long", rate, max_len, total);
                    if (piece == 0 && total != 0) return fail("empty piece", rate, max_len, total);
                    if (piece == rate && count != 0) return fail("a later piece of exactly one rate", rate, max_len, total);
                    done += piece;
                    ++count;
                } while (done < total);
                if (done != total) return fail("the pieces do not sum to the call", rate, max_len, total);
                ++cuts;
            }
        }
    for (size_t piece : {1, 2, 5})
        for (size_t longest = 0; longest <= 4 * piece + 2; ++longest) {
            const size_t n = longest + 1;   // row i has i elements; the caller's offsets start at 7
            std::vector<uint64_t> offsets(n + 1), off(n + 1), next(n, 0);
            offsets[0] = 7;
            for (size_t i = 0; i < n; ++i) offsets[i + 1] = offsets[i] + i;
            const size_t pieces = ragged_pieces(longest, piece);
            if (pieces != (longest + piece - 1) / piece) return fail("ragged_pieces", piece, longest, pieces);
            for (size_t p = 0; p < pieces; ++p) {
                ragged_offsets(offsets.data(), n, piece, p, off.data());
                if (off[0] != 0) return fail("offsets do not start at 0", piece, longest, p);
                for (size_t i = 0; i < n; ++i) {
                    const RowRange r = ragged_range(i, piece, p);
                    if (r.lo != next[i] || r.hi < r.lo || r.hi > i || r.hi - r.lo > piece) return fail("range out of order", piece, longest, i);
                    if (off[i + 1] - off[i] != r.hi - r.lo) return fail("offsets are not the running sums", piece, longest, i);
                    if (pieces == 1 && off[i + 1] != offsets[i + 1] - offsets[0]) return fail("one piece: not the caller's offsets", piece, longest, i);
                    next[i] = r.hi;
                }
            }
            for (size_t i = 0; i < n; ++i)
                if (next[i] != i) return fail("the pieces do not tile the row", piece, longest, i);
            ++raggeds;
        }
    std::printf("sanitized ok: %zu cuts, %zu ragged shapes\n", cuts, raggeds);
    return 0;
}
