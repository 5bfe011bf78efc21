// Host-side preparation of a validated config for the kernels: modulus view, conversion constants and the
// round constants / MDS matrix rewritten into the internal field form (29-bit limbs, x * 2^261 mod p).
// Shared by pmx_context.cpp (which uploads the table) and the CPU-side algorithm check in tests/hostcheck.
// The schedules themselves are derived in pmx_derive.hpp; this file lays them out: the serialisers, the table writer and prepare().
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "../../include/poseidon_mi355x.h"
#include "pmx_derive.hpp"
#include "pmx_field.hpp"
#include "pmx_host_field.hpp"
#include "pmx_permute.hpp"

namespace pmx {

inline void to_limbs29(const U256 &x, uint32_t out[kN]) {
    for (int i = 0; i < kN; ++i) {
        const int bit = kW * i, wi = bit / 64, sh = bit % 64;
        unsigned __int128 pair = x.l[wi];
        if (wi + 1 < 4) pair |= (unsigned __int128)x.l[wi + 1] << 64;
        out[i] = (uint32_t)(pair >> sh) & kMask;
    }
}

inline U256 times_pow2(const HostField &f, U256 v, int k) {  // v * 2^k mod p
    for (int i = 0; i < k; ++i) v = f.add(v, v);
    return v;
}

// an ABI Montgomery residue in the internal form: x*2^256 -> x*2^261
inline void to_internal(const HostField &f, const U256 &mont, uint32_t out[kN]) { to_limbs29(times_pow2(f, mont, 5), out); }

struct Prepared {
    HostField hf;
    FieldRt f;
    Fe one;                         // 2^261 mod p
    Rounds c;
    uint32_t t;
    // one table, kFeStride words per element, offsets in words:
    //   [0, mds_offset)            ark      [rounds][t]      dense schedule
    //   [mds_offset, opt_offset)   mds      [t][t]
    //   -- only when has_opt (see pmx_permute.hpp: OptTables) --
    //   opt_offset                 ark'     [rounds][t]
    //   -- t == 3 only: the element form of the optimised schedule's matrices, the source of the quad engine's table (coop) --
    //                              full     [RF-1][t][t]     one matrix per full round except the entrance round
    //                              sparse   [RP][2t-1]       layer 0 follows the entrance round, layer j partial round j-1
    //                              bdense   [t][t]           layer after the last partial round
    std::vector<uint32_t> consts;
    size_t mds_offset;
    bool has_opt;
    size_t opt_offset;
    //   -- only when has_opt and t == 3 (pmx_permute.hpp: cooperative schedule) --
    //   coop_offset                coop     [rounds][3][4]
    size_t coop_offset;
    //   -- only when mfma_dense: the dense layers as int8 GEMM operands (pmx_mfma.hpp); RF - 1 layers of `full`, then bdense --
    //   mfma_offset                [RF][mfma_layer_words(t)]
    size_t mfma_offset;
    bool mfma_dense;
    //   -- only when mfma_dense and mfma_window_for(t) > 0: the partial section as windows (pmx_mfma.hpp: mfma_window_words) --
    size_t win_offset;
    uint32_t mfma_window;   // K, or 0: no windows (the sparse layers run on the VALU)
    size_t io_offset;   // kIoWords words behind FieldRt::io
    bool unit_low_limb; // p = 1 mod 2^29: the window engines with the complemented quotient digits serve it (pmx_field.hpp: mont_sqr_p1)

    // the tables of the window engines in this (host) copy; valid while `consts` is neither copied nor resized
    OptTables opt_tables() const {
        OptTables tb;
        tb.ark = consts.data() + opt_offset;
        tb.mfma = consts.data() + mfma_offset;
        tb.win = consts.data() + win_offset;
        return tb;
    }
};

// balanced bytes of the 256-bit pattern v: digit e in [-128, 127], carry into the next; returns the carry out of digit 31
inline unsigned balanced_bytes(const U256 &v, int8_t out32[32]) {
    unsigned carry = 0;
    for (size_t e = 0; e < 32; ++e) {
        int dgt = (int)((v.l[e / 8] >> (8 * (e % 8))) & 0xff) + (int)carry;
        carry = 0;
        if (dgt >= 128) {
            dgt -= 256;
            carry = 1;
        }
        out32[e] = (int8_t)dgt;
    }
    return carry;
}

// The 32 bytes a residue Y is stored as.  32 balanced digits reach from -128 S to 127 S, S = (256^32 - 1) / 255: every residue of a modulus
// whose top byte is at most 126, but not the residues above 127 S = 0.996 * 2^255 of a larger one (2^255 - 19).  Such a residue Y is stored
// as Y - p instead (congruent, above -2^255 > -128 S: the digits of its two's-complement pattern, whose carry out is its sign).
// kStoredBroken: Y is no residue, or Y - p has no such digits (cannot happen: Y < p, and Y - p > -2^255 has 32 balanced digits).
enum StoredAs { kStoredPlain = 0, kStoredMinusP = 1, kStoredBroken = 2 };
inline StoredAs stored_bytes(const HostField &hf, const U256 &y, int8_t out32[32]) {
    if (u256_geq(y, hf.p)) return kStoredBroken;
    if (!balanced_bytes(y, out32)) return kStoredPlain;
    U256 neg;
    const uint64_t borrow = u256_sub(neg, y, hf.p);
    const unsigned sign = balanced_bytes(neg, out32);
    return borrow && sign ? kStoredMinusP : kStoredBroken;
}

// One dense layer as the A operands of pmx_mfma.hpp: `rows` = t rows of t constants (ABI Montgomery residues, row-major).
// Row i, k-step q, lane l: 16 bytes = bytes e = l & 31 of the residues  Y = c_ij * 2^(8 b + 24) mod p  for the 16 positions
// k = 32 q + 16 (l >> 5) + 0..15 of the state's byte string (k = 32 j + b), as balanced signed bytes; then per row the eight
// word sums of 128 * sum_k Y_k (the state's bytes enter as u - 128).
// General form: n_out rows of n_in constants; aff (may be null): one constant per row added to the row's value.
// (the table carries the 2^24 the row's finish divides by - element or operand form, the Montgomery step is the same: pmx_mfma.hpp, mfma_row_acc)
// A residue stored as Y - p (stored_bytes) makes the row's correction take 255 p for it - the term then contributes U Y + (255 - U) p for
// the state byte U in [0, 255]: non-negative, congruent, and at most 255 p like every other term, so every bound of pmx_mfma.hpp stands as
// it is (round 6; until then those moduli had no tables and ran on VALU rows).
// Returns false, with the layer half written, if a residue has no stored form (stored_bytes: an invariant of this file is broken).
inline bool put_mfma_layer_io(const HostField &hf, const U256 *rows, size_t n_in, size_t n_out, const U256 *aff, uint32_t *dst) {
    const size_t nq = (size_t)mfma_k_steps((int)n_in), row_words = (size_t)mfma_row_words((int)n_in);
    int8_t *bytes = reinterpret_cast<int8_t *>(dst);
    long long *corr = reinterpret_cast<long long *>(dst + n_out * row_words);
    for (size_t i = 0; i < n_out; ++i) {
        long long colsum[32] = {0};
        size_t negatives = 0;
        constexpr int shift = kMfmaShift;
        for (size_t j = 0; j < n_in; ++j) {
            U256 y = times_pow2(hf, hf.from_mont(rows[i * n_in + j]), shift);
            for (size_t b = 0; b < (size_t)kMfmaElemBytes; ++b) {   // (the inputs of a layer are below 2^256: pmx_mfma.hpp)
                const size_t k = j * kMfmaElemBytes + b, q = k / 32, r = k % 32, h = r / 16, byte = r % 16;
                int8_t d32[32];
                const StoredAs as = stored_bytes(hf, y, d32);
                if (as == kStoredBroken) return false;
                if (as == kStoredMinusP) ++negatives;
                for (size_t e = 0; e < 32; ++e) {
                    bytes[(((i * nq + q) * 64 + 32 * h + e) * 16) + byte] = d32[e];
                    colsum[e] += d32[e];
                }
                y = times_pow2(hf, y, 8);
            }
        }
        // the row's constant in the units of V: its internal form (x 2^261) times the 2^kMfmaShift the finish divides by
        U256 add = {{0, 0, 0, 0}};
        if (aff) add = times_pow2(hf, hf.from_mont(aff[i]), 261 + shift);
        for (size_t w = 0; w < 8; ++w) {
            long long v = 0;
            for (size_t tt = 0; tt < 4; ++tt) v += (128 * colsum[4 * w + tt]) * (1ll << (8 * tt));
            const long long p_word = (long long)((hf.p.l[w / 2] >> (32 * (w % 2))) & 0xffffffffull);   // (negatives * 255 < 2^18: the product stays below 2^50)
            corr[i * 8 + w] = v + (long long)((add.l[w / 2] >> (32 * (w % 2))) & 0xffffffffull) + (long long)(negatives * 255) * p_word;
        }
    }
    return true;
}
inline bool put_mfma_layer(const HostField &hf, const U256 *rows, size_t t, uint32_t *dst) { return put_mfma_layer_io(hf, rows, t, t, nullptr, dst); }

// shifted table of a ROW of n constants (given as ABI Montgomery residues C_i * 2^256) in the chunked layout of
// pmx_field.hpp (tab_index): limb k of C_i * 2^(29 j + 58) mod p; tab_row_words(n) words, padding left 0
inline void put_shifted_row(const HostField &hf, const U256 *c_mont, size_t n, uint32_t *tab) {
    for (size_t i = 0; i < n; ++i) {
        U256 tj = times_pow2(hf, hf.from_mont(c_mont[i]), 58);
        for (int j = 0; j < kN; ++j) {
            uint32_t limbs[kN];
            to_limbs29(tj, limbs);
            for (int k = 0; k < kN; ++k) {
                const size_t ng = (n + kTabChunk - 1) / kTabChunk;
                const size_t at = n == 1 ? (size_t)(k / kTabChunk) * kTabChunkWords + (k % kTabChunk) * kN + j
                                         : ((size_t)k * ng + i / kTabChunk) * kTabChunkWords + (i % kTabChunk) * kN + j;
                tab[at] = limbs[k];
            }
            tj = times_pow2(hf, tj, kW);
        }
    }
}

// The table as it grows: a section begins where the writer stands, and every word of the layout is appended through it.  `grow` may move
// the table: what it returns is an index, and a pointer made from one is not kept across the next call.
struct TableWriter {
    std::vector<uint32_t> &words;
    const HostField &hf;
    size_t at() const { return words.size(); }                                    // where the next word goes
    size_t grow(size_t n) { words.resize(at() + n, 0u); return at() - n; }        // n zero words: where they start
    void align16() { grow((4 - at() % 4) % 4); }                                  // 16-byte operands
    void put(const U256 &mont) { const size_t k = grow(kFeStride); to_internal(hf, mont, &words[k]); }   // one element, an ABI Montgomery residue
    void truncate(size_t mark) { words.resize(mark); }                            // back to an earlier at()
};

// What the stages of prepare() share, all as ABI Montgomery residues.
struct Schedules {
    std::vector<U256> ark;                                                        // the config's own: [rounds][t]
    HostMat M;
    std::vector<U256> ark_opt, full, sparse, bdense, entrance_scale, exit_scale;  // derive_opt_tables, when Prepared::has_opt
};

inline int layer_failed(std::string &err, const std::string &layer) {
    err = "int8 table of " + layer + ": a constant has no 32 balanced bytes (host invariant broken)";
    return PMX_ERR_HOST;
}

// ---- the stages of prepare(), one per section of the layout (Prepared) ------------------------------------------------------------------
// the limits of this build on shape and modulus, and every constant a reduced residue (ark-ff's invariant); reads the constants into `s`
inline int prepare_validate(const pmx_config *cfg, Prepared &out, Schedules &s, std::string &err) {
    const uint64_t t64 = (uint64_t)cfg->rate + cfg->capacity;
    if (cfg->rate == 0) { err = "rate must be >= 1"; return PMX_ERR_CONFIG; }
    if (t64 > PMX_MAX_WIDTH) { err = "width exceeds PMX_MAX_WIDTH"; return PMX_ERR_UNSUPPORTED; }
    const uint64_t rounds = (uint64_t)cfg->full_rounds + cfg->partial_rounds;
    if (rounds == 0 || rounds > 4096) { err = "round count out of range"; return PMX_ERR_CONFIG; }
    HostField &hf = out.hf;
    if (!hf.init(cfg->modulus)) { err = "modulus must be odd and > 2"; return PMX_ERR_CONFIG; }
    // the unsaturated 9 x 29-bit arithmetic needs 6 spare bits below 2^261 (pmx_field.hpp)
    if (hf.bits() > 255) { err = "modulus must be < 2^255 (BLS12-381 Fr and BN254 Fr are 255 and 254 bits)"; return PMX_ERR_UNSUPPORTED; }
    if (hf.bits() < 225) { err = "modulus must be at least 225 bits"; return PMX_ERR_UNSUPPORTED; }
    const uint32_t t = out.t = (uint32_t)t64;
    const size_t n_ark = (size_t)rounds * t, n_mds = (size_t)t * t;
    s.ark.resize(n_ark);
    s.M.assign(t, std::vector<U256>(t));
    for (size_t k = 0; k < n_ark + n_mds; ++k) {
        const bool is_ark = k < n_ark;
        const size_t i = is_ark ? k : k - n_ark;
        U256 &v = is_ark ? s.ark[i] : s.M[i / t][i % t];
        std::memcpy(v.l, (is_ark ? cfg->ark : cfg->mds) + 4 * i, sizeof v.l);
        if (u256_geq(v, hf.p)) {
            err = std::string(is_ark ? "ark" : "mds") + " constant " + std::to_string(i) + " is not reduced";
            return PMX_ERR_CONFIG;
        }
    }
    return PMX_OK;
}

inline void put_dense_schedule(TableWriter &tw, const Schedules &s, Prepared &out) {
    for (const U256 &v : s.ark) tw.put(v);
    out.mds_offset = tw.at();
    for (const auto &row : s.M)
        for (const U256 &v : row) tw.put(v);
}

// ark' for every engine of the optimised schedule; the matrices in element form only where the quad engine's table is built from them
// (t = 3) - the window engines read the same matrices as int8 tables (put_dense_layers)
inline void put_opt_schedule(const pmx_config *cfg, TableWriter &tw, Schedules &s, Prepared &out) {
    const HostField &hf = out.hf;
    long double pv = 0;
    for (int i = 3; i >= 0; --i) pv = pv * 18446744073709551616.0L + (long double)hf.p.l[i];
    long double two_261 = 1;
    for (int i = 0; i < 261; ++i) two_261 *= 2;
    const uint32_t rounds = cfg->full_rounds + cfg->partial_rounds;
    out.has_opt = opt_schedule_lane_headroom(two_261 / pv, cfg->partial_rounds, cfg->alpha) &&
                  derive_opt_tables(hf, out.t, cfg->full_rounds / 2, cfg->partial_rounds, rounds, cfg->alpha, s.ark, s.M, s.ark_opt, s.full, s.sparse,
                                    s.bdense, &s.entrance_scale, &s.exit_scale);
    out.opt_offset = tw.at();
    if (!out.has_opt) return;
    for (const U256 &v : s.ark_opt) tw.put(v);
    if (out.t == 3)
        for (const auto *vec : {&s.full, &s.sparse, &s.bdense})
            for (const U256 &v : *vec) tw.put(v);
}

// cooperative t = 3 table: per (round, lane): ark' element, then the lane's matrix row of that round
inline void put_coop_table(const pmx_config *cfg, TableWriter &tw, const Schedules &s, Prepared &out) {
    out.coop_offset = tw.at();
    if (!out.has_opt || out.t != 3) return;
    const size_t half = cfg->full_rounds / 2, rp = cfg->partial_rounds, rounds = (size_t)cfg->full_rounds + rp;
    tw.grow(rounds * 3 * kCoopElems * kFeStride);
    auto put = [&](size_t r, size_t q, size_t slot, const U256 &v) {
        to_internal(out.hf, v, &tw.words[out.coop_offset + ((r * 3 + q) * kCoopElems + slot) * kFeStride]);
    };
    const bool folded = cfg->alpha == 5 || cfg->alpha == 17;   // folded sparse rounds (pmx_permute.hpp: coop_fold_*)
    for (size_t r = 0; r < rounds; ++r) {
        const bool partial = r >= half && r < half + rp;
        for (size_t q = 0; q < 3; ++q) {
            put(r, q, 0, s.ark_opt[r * 3 + q]);
            if (r + 1 == half || (partial && r + 1 < half + rp)) {       // sparse layer: row0[3] = (ONE, v_1, v_2), w[2]
                const U256 *sp = &s.sparse[(r + 1 - half) * 5];
                if (partial && folded) {
                    if (q == 0) {
                        put(r, q, 1, sp[0]);                          // stage A: x * ONE
                    } else {
                        put(r, q, 1, sp[3 + q - 1]);                  // stage A: x * w_q
                        put(r, q, 2, sp[q]);                          // stage B: s_q * v_q
                    }
                } else if (q == 0) {                                  // uniform rounds (the entrance round is one: full S-box layer)
                    for (size_t j = 0; j < 3; ++j) put(r, q, 1 + j, sp[j]);
                } else {
                    put(r, q, 1, sp[3 + q - 1]);                      // w_q * z_0
                    put(r, q, 1 + q, out.hf.r);                       // + ONE * z_q   (other slot stays 0)
                }
            } else {
                const U256 *mat = partial ? s.bdense.data() : &s.full[full_matrix_ordinal((uint32_t)r, (uint32_t)half, (uint32_t)rp) * 9];
                for (size_t j = 0; j < 3; ++j) put(r, q, 1 + j, mat[q * 3 + j]);
            }
        }
    }
}

// the dense layers as int8 GEMM operands
inline int put_dense_layers(const pmx_config *cfg, TableWriter &tw, const Schedules &s, Prepared &out, std::string &err) {
    tw.align16();
    out.mfma_offset = tw.at();
    const uint32_t t = out.t;
    const size_t n_full = cfg->full_rounds ? (size_t)cfg->full_rounds - 1 : 0;   // matrices in `full`
    // (a layer's inputs must be below 2^256: S-box outputs ARE products for every alpha - pmx_field.hpp: fe_sbox; p < 2^255 is a limit of the build)
    out.mfma_dense = out.has_opt && t >= PMX_MFMA_MIN_T && t <= PMX_MFMA_MAX_T && n_full >= 1;
    if (!out.mfma_dense) return PMX_OK;
    for (size_t o = 0; o <= n_full; ++o) {
        const U256 *rows = o < n_full ? &s.full[o * t * t] : s.bdense.data();
        const size_t k = tw.grow((size_t)mfma_layer_words((int)t));
        if (!put_mfma_layer(out.hf, rows, t, &tw.words[k])) return layer_failed(err, "dense layer " + std::to_string(o));
    }
    return PMX_OK;
}

// ... and the partial section as windows closed by one such layer each, with one constant behind them.  A width that takes windows has no
// sparse layers in its matrix-core kernels: if the windows cannot be derived (a zero where the algebra divides) the config runs on the VALU
// rows - the dense layers leave the table again.
inline int put_windows(const pmx_config *cfg, TableWriter &tw, const Schedules &s, Prepared &out, std::string &err) {
    const HostField &hf = out.hf;
    const uint32_t t = out.t, half = cfg->full_rounds / 2, rp = cfg->partial_rounds;
    out.win_offset = tw.at();
    out.mfma_window = 0;
    if (!out.mfma_dense || mfma_window_for((int)t) <= 0) return PMX_OK;
    const uint32_t K = (uint32_t)mfma_window_for((int)t);
    WindowPlan plan;
    if (K > t || !derive_window_layers(hf, t, half, rp, cfg->alpha, K, s.ark, s.M, s.entrance_scale, s.exit_scale, &s.ark_opt[(size_t)(half + rp) * t], plan)) {
        out.mfma_dense = false;
        tw.truncate(out.mfma_offset);
        out.win_offset = tw.at();
        return PMX_OK;
    }
    const size_t nh = (size_t)mfma_window_hist((int)K);
    // (rows that only feed matrix-core inputs - every carried lane but the first, where the history terms are rows too - stay in
    // operand form between the layers: pmx_mfma.hpp, mfma_fe_rows; the last window's layer feeds S-boxes on every lane)
    size_t k = tw.grow((size_t)mfma_layer_words((int)t));
    if (!put_mfma_layer_io(hf, plan.entry_rows.data(), t, t, plan.entry_aff.data(), &tw.words[k])) return layer_failed(err, "the windows' entry layer");
    for (size_t w = 0; w < plan.n_win; ++w) {
        k = tw.grow((size_t)mfma_layer_words_io((int)(t - 1 + K), (int)t));
        if (!put_mfma_layer_io(hf, plan.rows[w].data(), t - 1 + K, t, plan.aff[w].data(), &tw.words[k])) return layer_failed(err, "window layer " + std::to_string(w));
        const size_t h = tw.grow((size_t)mfma_window_hist_words((int)t, (int)K));
        for (uint32_t j = 2; j < K; ++j) {
            const U256 *hist = &plan.hist[w * nh + (size_t)mfma_window_hist((int)j)];
            if (!mfma_hist_tab((int)t)) {   // the history terms as matrix-core rows: the row of x_{j+1} over (z_1 .. z_{j-1}, u_j), coefficients (h_{j,.}, ONE)
                std::vector<U256> row(hist, hist + (j - 1));
                row.push_back(hf.r);
                if (!put_mfma_layer_io(hf, row.data(), j, 1, nullptr, &tw.words[h + mfma_hist_rows_offset((int)j)]))
                    return layer_failed(err, "the history rows of window " + std::to_string(w));
            } else if (j == 2 && plan.hist_small[w]) {   // h_{2,1} = 1 .. 4: no table - a marker no limb can be, and the integer (pmx_permute.hpp)
                tw.words[h + mfma_hist_tab_offset(2)] = kMfmaHistSmallMarker;
                tw.words[h + mfma_hist_tab_offset(2) + 1] = plan.hist_small[w];
            } else {
                put_shifted_row(hf, hist, j - 1, &tw.words[h + mfma_hist_tab_offset((int)j)]);
            }
        }
    }
    // behind the windows: S-box(ark'[0][0]) - what lane 0 of round 0 is when that lane comes in as zero (the capacity lane of a fresh
    // sponge: every 2-to-1 compression, the first permutation of every hash row), so those kernels skip that S-box (pmx_permute.hpp)
    tw.put(hf.pow(s.ark_opt[0], cfg->alpha));
    out.mfma_window = K;
    return PMX_OK;
}

// the run-time view of the field, with the constants of the ABI conversions (FieldRt::io) in the table
inline void put_field_block(TableWriter &tw, Prepared &out) {
    const HostField &hf = out.hf;
    FieldRt &f = out.f;
    f.unit = 1;
    to_limbs29(hf.p, f.p);
    f.pinv = (uint32_t)hf.inv & kMask;
    out.unit_low_limb = field_unit_low_limb(f.p);
    out.io_offset = tw.grow(kIoWords);
    uint32_t *io = &tw.words[out.io_offset];
    std::memcpy(io + kIoP32, hf.p.l, 32);
    to_limbs29(times_pow2(hf, hf.r, 10), io + kIoToInt);   // 2^266 mod p
    to_limbs29(hf.r, io + kIoToAbi);                       // 2^256 mod p
    to_internal(hf, hf.r2, io + kIoFromU64);               // 2^517 mod p
    f.io = io;   // host view; valid while `out` is neither copied nor resized
    to_internal(hf, hf.r, out.one.l);                      // 2^261 mod p
}

inline void put_rounds(const pmx_config *cfg, Prepared &out) {
    out.c.rate = cfg->rate;
    out.c.capacity = cfg->capacity;
    out.c.half_full = cfg->full_rounds / 2;   // odd RF: RF/2 full rounds before the partial section, RF - RF/2 after (mod.rs:96-116)
    out.c.partial_rounds = cfg->partial_rounds;
    out.c.total_rounds = cfg->full_rounds + cfg->partial_rounds;
    out.c.alpha = cfg->alpha;
}

// Returns PMX_OK or an error code with a message in `err`.
inline int prepare(const pmx_config *cfg, Prepared &out, std::string &err) {
    Schedules s;
    int rc = prepare_validate(cfg, out, s, err);
    if (rc) return rc;
    out.consts.clear();
    TableWriter tw{out.consts, out.hf};
    put_dense_schedule(tw, s, out);
    put_opt_schedule(cfg, tw, s, out);
    put_coop_table(cfg, tw, s, out);
    if ((rc = put_dense_layers(cfg, tw, s, out, err)) != PMX_OK) return rc;
    if ((rc = put_windows(cfg, tw, s, out, err)) != PMX_OK) return rc;
    put_field_block(tw, out);
    put_rounds(cfg, out);
    return PMX_OK;
}

}  // namespace pmx
