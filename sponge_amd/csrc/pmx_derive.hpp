// The two schedule derivations the host does at context creation, on the config's constants in the ABI Montgomery form: the optimised
// schedule (derive_opt_tables) and the partial section as windows (derive_window_layers).  pmx_prepare.hpp serialises what they return.
#pragma once
#include <vector>

#include "pmx_host_field.hpp"
#include "pmx_host_mat.hpp"
#include "pmx_mfma.hpp"

namespace pmx {

// The optimised schedule updates its identity lanes without a magnitude cap (pmx_permute.hpp: mont_mul_add).
// With Q = 2^261 / p (>= 64) and every lane below Q p (nine normalised limbs), row 0 of a sparse layer returns at most
// (t-1) + B_z + 1 <= 10.3 p for t <= 9, so the S-box input x = row0 + constant is below 11.3 p and the S-box output z_0
// below B_z p with
//     alpha >= 4: the chain ends in a product with x of a value < 1.05 p  ->  B_z < 1.05 * 11.3 / 64 + 1 < 1.2
//     alpha = 3: x^2 * x, x^2 < 3 p -> B_z < 1.6;   alpha = 2: B_z < 3;   alpha = 1: z_0 = x as the product x * 1 (fe_sbox), B_z < 1.2;
//     alpha = 0: z_0 = 1.
// A lane starts as an S-box output of the entrance round (< 1.3 p), takes its first update there and one more per sparse
// partial round, growing by at most (B_z / Q + 1) p each time; the dense layer after the last partial round adds its own
// + p.  The schedule is used when all of that stays below Q.
inline bool opt_schedule_lane_headroom(long double two_261_over_p, uint32_t partial_rounds, uint64_t alpha) {
    const long double bz = alpha == 0 ? 1.0L : alpha == 2 ? 3.0L : alpha == 3 ? 1.6L : 1.3L;
    const long double growth = 1.0L + bz / two_261_over_p;
    const long double worst = 1.4L + growth * (long double)partial_rounds + 1.5L;
    return worst < two_261_over_p;
}

// index of a full round's matrix in the `full` table: every full round but the entrance round (the last one of the first
// half, whose linear layer is sparse[0]) has its own, in round order
inline size_t full_matrix_ordinal(uint32_t r, uint32_t half_full, uint32_t rp) { return r < half_full ? r : r - rp - 1; }

// Derives the tables of the optimised schedule from (ark, mds).  Two exact rewrites of the same permutation:
//
// (1) Basis change on lanes 1..t-1 (Poseidon paper, appendix B).  The partial rounds apply no S-box to those lanes, so they
//     may be carried in any basis N_j = diag(1, Nh_j).  With B_j = M N_j the layer after S-box layer j becomes
//     sparse_j = N_{j+1}^-1 B_j = [[b00, bv], [Bh^-1 bw, I]]  for Nh_{j+1} = Bh_j (lower-right block of B_j): 2t-1 products
//     instead of t^2.  Layer j = 0 is the one after the LAST FULL ROUND OF THE FIRST HALF (the "entrance" round: the state
//     it produces is only ever used in the new basis), j = 1..RP-1 follow the partial rounds, and the layer after the last
//     partial round is dense (B_RP: the full rounds need every lane back).  Round constants of lanes 1.. are deferred
//     (vector D) and re-enter through lane 0 (e_j) and through the first full round after the partial section.
//
// (2) Diagonal scalings.  x -> x^alpha commutes with a diagonal matrix up to its alpha-th power, S(D x) = D^alpha S(x), so
//     the state between two rounds may be carried as D_r s_r for any invertible diagonal D_r (the same D at both ends): every
//     constant is rescaled on the host, nothing else changes.  One free scalar per lane and round boundary makes one matrix
//     entry per row equal to ONE: column 0 of every dense layer that feeds a full S-box layer, the coefficient of the
//     S-box output in row 0 of every sparse layer (the lanes keep their unit coefficients).  A normalised row is
//     z_0 + sum_{j >= 1} c_j z_j: t-1 products and an addend.  Only the last round's matrix stays fully dense (its
//     output is the permutation's, unscaled).
//
// Products by constants per permutation: (RF-2) t (t-1) + t^2 + RP (2t-2) + t (t-1), e.g. t = 3, 8 + 31: 175 (dense
// schedule 351); t = 9, 8 + 57: 1497 (5265).
inline bool derive_opt_tables(const HostField &f, uint32_t t, uint32_t half_full, uint32_t rp, uint32_t rounds, uint64_t alpha,
                              const std::vector<U256> &ark, const HostMat &M, std::vector<U256> &ark_opt,
                              std::vector<U256> &fullmat, std::vector<U256> &sparse, std::vector<U256> &bdense,
                              std::vector<U256> *entrance_scale = nullptr, std::vector<U256> *exit_scale = nullptr) {
    if (rp == 0 || half_full == 0 || t < 2 || half_full + rp >= rounds) return false;
    const size_t n = t - 1, per = 2 * (size_t)t - 1;
    const uint32_t rf_total = rounds - rp, entrance = half_full - 1, last_partial = half_full + rp - 1;
    const U256 zero = {{0, 0, 0, 0}};
    // ---- (1) basis change ----------------------------------------------------------------------------------------
    ark_opt = ark;
    sparse.assign((size_t)rp * per, zero);
    HostMat Nh = mat_identity(f, n);
    HostMat B;
    std::vector<U256> D(n, zero);   // deferred constants of lanes 1.., in the current basis
    for (uint32_t j = 0; j <= rp; ++j) {
        // B = M * diag(1, Nh)
        B.assign(t, std::vector<U256>(t, zero));
        for (size_t i = 0; i < t; ++i) {
            B[i][0] = M[i][0];
            for (size_t c = 0; c < n; ++c)
                for (size_t l = 0; l < n; ++l) B[i][1 + c] = f.add(B[i][1 + c], f.mul(M[i][1 + l], Nh[l][c]));
        }
        if (j == rp) break;
        HostMat Bh(n, std::vector<U256>(n)), Bh_inv;
        for (size_t i = 0; i < n; ++i)
            for (size_t c = 0; c < n; ++c) Bh[i][c] = B[1 + i][1 + c];
        if (!mat_inverse(f, Bh, Bh_inv)) return false;
        U256 *sp = &sparse[(size_t)j * per];
        for (size_t c = 0; c < t; ++c) sp[c] = B[0][c];                  // row0 = (b00, bv)
        std::vector<U256> bw(n);
        for (size_t i = 0; i < n; ++i) bw[i] = B[1 + i][0];
        const std::vector<U256> w = mat_vec(f, Bh_inv, bw);              // Bh^-1 bw
        for (size_t i = 0; i < n; ++i) sp[t + i] = w[i];
        // constants of the round that follows (partial round j) in the new basis
        const size_t rn = (size_t)(half_full + j) * t;
        std::vector<U256> c1(n);
        for (size_t i = 0; i < n; ++i) c1[i] = ark[rn + 1 + i];
        const std::vector<U256> ct = mat_vec(f, Bh_inv, c1);
        U256 e = ark[rn];
        for (size_t c = 0; c < n; ++c) e = f.add(e, f.mul(B[0][1 + c], D[c]));   // + bv . D
        ark_opt[rn] = e;
        for (size_t i = 0; i < n; ++i) { ark_opt[rn + 1 + i] = zero; D[i] = f.add(D[i], ct[i]); }
        Nh = Bh;
    }
    bdense.assign((size_t)t * t, zero);
    for (size_t i = 0; i < t; ++i)
        for (size_t c = 0; c < t; ++c) bdense[i * t + c] = B[i][c];
    // E = B [0; D] joins the constants of the first full round after the partial section
    const size_t rf = (size_t)(half_full + rp) * t;
    for (size_t i = 0; i < t; ++i) {
        U256 e = zero;
        for (size_t c = 0; c < n; ++c) e = f.add(e, f.mul(B[i][1 + c], D[c]));
        ark_opt[rf + i] = f.add(ark[rf + i], e);
    }
    fullmat.assign((size_t)(rf_total - 1) * t * t, zero);
    for (size_t o = 0; o + 1 < rf_total; ++o)
        for (size_t i = 0; i < t; ++i)
            for (size_t c = 0; c < t; ++c) fullmat[(o * t + i) * t + c] = M[i][c];
    // ---- (2) diagonal scalings -------------------------------------------------------------------------------------
    // D at both ends of the permutation is 2^-5, not 1: the internal form of x / 32 is (x / 32) 2^261 = x 2^256, the ABI
    // residue itself, so states, absorbed and squeezed elements enter and leave the kernels without a multiplication
    // (pmx_field.hpp: fe_from_abi_scaled / fe_to_abi_scaled).  Between two permutations of a sponge the state stays in
    // these coordinates.
    const U256 thirty_two = {{32, 0, 0, 0}};
    const U256 io_scale = f.inverse(f.to_mont(thirty_two));
    std::vector<U256> d(t, io_scale), dn(t), e(t), inv_e(t);
    for (uint32_t r = 0; r < rounds; ++r) {
        const bool full = r < half_full || r > last_partial;
        for (size_t i = 0; i < t; ++i) ark_opt[(size_t)r * t + i] = f.mul(ark_opt[(size_t)r * t + i], d[i]);   // D_r c_r
        for (size_t i = 0; i < t; ++i) {                // scaling of what enters the linear layer
            e[i] = (full || i == 0) ? f.pow(d[i], alpha) : d[i];
            if (u256_is_zero(e[i])) return false;
            inv_e[i] = f.inverse(e[i]);
        }
        if (r == entrance && entrance_scale) *entrance_scale = e;       // what multiplies the S-box outputs of the entrance round
        if (r == last_partial + 1 && exit_scale) *exit_scale = d;       // what multiplies the state that enters the first full round after the partial section
        if (r == entrance || (!full && r < last_partial)) {            // sparse layer
            U256 *sp = &sparse[(size_t)(r - entrance) * per];
            if (u256_is_zero(sp[0])) return false;
            dn[0] = f.mul(e[0], f.inverse(sp[0]));
            for (size_t c = 1; c < t; ++c) sp[c] = f.mul(f.mul(sp[c], dn[0]), inv_e[c]);
            sp[0] = f.r;                                               // the coefficient of the S-box output: one
            for (size_t i = 1; i < t; ++i) {
                dn[i] = e[i];                                          // the lanes keep their unit coefficients
                sp[t + i - 1] = f.mul(f.mul(sp[t + i - 1], dn[i]), inv_e[0]);
            }
        } else {
            const bool last = r + 1 == rounds;
            U256 *L = full ? &fullmat[full_matrix_ordinal(r, half_full, rp) * t * t] : bdense.data();
            for (size_t i = 0; i < t; ++i) {
                if (last) {
                    dn[i] = io_scale;
                } else {
                    if (u256_is_zero(L[i * t])) return false;
                    dn[i] = f.mul(e[0], f.inverse(L[i * t]));          // column 0 becomes one
                }
                for (size_t c = 0; c < t; ++c) L[i * t + c] = f.mul(f.mul(L[i * t + c], dn[i]), inv_e[c]);
                if (!last) L[i * t] = f.r;
            }
        }
        d = dn;
    }
    return true;
}

// ---- the partial section as windows (pmx_mfma.hpp, pmx_permute.hpp: MFMA_WINDOW) ----------------------------------------------
// Exact algebra on the reference's rounds (s <- M (s + c_r with lane 0 raised to alpha)), per window of kw <= K partial rounds:
// with sigma = lanes 1.. of the true state at the window's start and z_1 .. z_kw its S-box outputs, every later S-box input and the
// state at the window's end are affine in (sigma, z).  The window carries  x^_1 = x_1  and  u^ = Psi sigma + psi  where the first
// kw - 1 rows of Psi are the sigma-parts (and constants) of x_2 .. x_kw, scaled by delta_{k+1} = delta_k^alpha / M_00 so that
//     x^_{k+1} = delta_{k+1} x_{k+1} = z^_k + u^_k + sum_{i<k} h_{k,i} z^_i,      z^_k = x^_k^alpha = delta_k^alpha z_k,
// and the other rows are unit rows that keep Psi invertible.  Layer w maps (u^, z^) of window w to (x^_1, u^) of window w + 1 (the
// last one to what the first full round after the section expects: D (s + c) minus the constant the kernel adds there), the entry
// layer maps the scaled S-box outputs of the entrance round to window 0.
struct WindowPlan {
    size_t n_win = 0;
    std::vector<U256> entry_rows, entry_aff;                 // t x t, t
    std::vector<std::vector<U256>> rows, aff;                // per window: t x (t - 1 + K), t
    std::vector<U256> hist;                                  // per window mfma_window_hist(K) constants
    std::vector<uint32_t> hist_small;                        // per window: h_{2,1} as a small integer (1 .. 4), or 0 (derive_window_layers: the window's free scale)
};

// ---- a window's free scale ------------------------------------------------------------------------------------------
// x^_1 of a window may be carried scaled by any lambda (the layer in front multiplies row 0 by it): the single history constant of a
// window of three S-boxes becomes h lambda^(alpha^2 - alpha), and where s / h has such a root for a small integer s the product h z^_1
// - 81 + 18 multiplies from a shifted table - is s lazy additions (pmx_permute.hpp).  alpha = 5: 20 = 5 * 4 and gcd(5, p - 1) = 1 for
// a config whose S-box is a permutation - a fifth root always exists, a fourth root for one value in four; alpha = 17: one in sixteen.
// lambda with lambda^(alpha (alpha - 1)) = y, or false: the alpha-th root and the odd part of alpha - 1 by inverting the exponent, the
// power of two in alpha - 1 by square roots (alpha = 5: 20 = 5 * 4, alpha = 17: 272 = 17 * 16, alpha = 257: 257 * 256)
inline bool host_root_window_scale(const HostField &f, const U256 &y, uint64_t alpha, U256 &lambda) {
    if (alpha < 2 || alpha > ((uint64_t)1 << 32)) return false;
    uint64_t m = alpha - 1;
    unsigned a = 0;
    while (!(m & 1)) {
        m >>= 1;
        ++a;
    }
    U256 u;
    if (!host_root_coprime(f, y, alpha, u) || !host_root_coprime(f, u, m, u)) return false;
    if (!host_is_2power_residue(f, u, a)) return false;
    for (unsigned left = a; left > 0; --left) {            // of the two square roots the one that is still a 2^(left-1)-th power
        U256 r;
        if (!host_sqrt(f, u, r)) return false;
        if (!host_is_2power_residue(f, r, left - 1)) r = f.neg(r);
        if (!host_is_2power_residue(f, r, left - 1)) return false;
        u = r;
    }
    lambda = u;
    U256 chk = f.pow(f.pow(lambda, alpha), alpha - 1);
    return u256_eq(chk, y);
}

typedef std::vector<U256> Form;   // an affine form over a window's generators: sigma (t - 1), z_1 .. z_K, and last (index G) the constant

// One window of derive_window_layers.
struct Window {
    uint32_t kw = 0, first_round = 0;     // its partial rounds (K; the first window takes what is left over) and the first of them
    std::vector<Form> X, Send;            // the S-box inputs x_2 .. x_kw (by index) and the true state after the window, over (sigma, z, 1)
    U256 lane0;                           // delta_1 of the window: x^_1 = lane0 x_1 (1 unless a better one exists: window_choose_scale)
    // what the layer BEFORE the window has to produce, from the true state at the window's start: x^_1 = s_0 + c, u^ = Psi s_1.. + psi
    HostMat Psi, PsiInv;
    std::vector<U256> psi;
    std::vector<U256> zscale;             // delta_j^-alpha: z_j = zscale_j z^_j
};

// the S-box inputs and the end state of a window as affine forms in (sigma, z)
inline void window_affine_forms(const HostField &f, uint32_t t, uint32_t K, const std::vector<U256> &ark, const HostMat &M, Window &win) {
    const U256 zero = {{0, 0, 0, 0}};
    const size_t n = t - 1, G = n + K;                       // generators: sigma (n), z_1..z_K; index G = the constant
    auto unit = [&](size_t g) { Form v(G + 1, zero); v[g] = f.r; return v; };
    std::vector<Form> S(t, Form(G + 1, zero));
    win.X.assign(win.kw + 1, Form());
    for (size_t i = 1; i < t; ++i) S[i] = unit(i - 1);
    for (uint32_t j = 1; j <= win.kw; ++j) {
        const U256 *c = &ark[(size_t)(win.first_round + j - 1) * t];
        std::vector<Form> y = S;
        for (size_t i = 0; i < t; ++i) y[i][G] = f.add(y[i][G], c[i]);
        if (j >= 2) win.X[j] = y[0];
        y[0] = unit(n + j - 1);
        for (size_t i = 0; i < t; ++i) {
            Form acc(G + 1, zero);
            for (size_t l = 0; l < t; ++l)
                for (size_t g = 0; g <= G; ++g)
                    if (!u256_is_zero(y[l][g])) acc[g] = f.add(acc[g], f.mul(M[i][l], y[l][g]));
            S[i] = acc;
        }
    }
    win.Send = S;
}

// the scales of the S-box inputs, x^_j = delta_j x_j, for a given delta_1 (the window's free scale); `hist`: the window's
// mfma_window_hist(K) history constants
inline bool window_scales(const HostField &f, uint32_t t, uint32_t K, uint64_t alpha, const U256 &delta1, Window &win, U256 *hist) {
    const U256 zero = {{0, 0, 0, 0}};
    const size_t n = t - 1, G = n + K;
    const uint32_t kw = win.kw;
    std::vector<U256> delta(kw + 1, f.r), dpow(kw + 1, f.r);   // delta_j, delta_j^alpha
    delta[1] = delta1;
    dpow[1] = f.pow(delta1, alpha);
    if (u256_is_zero(dpow[1])) return false;
    win.zscale.assign(K, zero);
    win.zscale[0] = f.inverse(dpow[1]);
    win.Psi.assign(n, std::vector<U256>(n, zero));
    win.psi.assign(n, zero);
    for (uint32_t j = 2; j <= kw; ++j) {
        const U256 a = win.X[j][n + j - 2];              // coefficient of z_{j-1} in x_j
        if (u256_is_zero(a)) return false;
        delta[j] = f.mul(dpow[j - 1], f.inverse(a));
        dpow[j] = f.pow(delta[j], alpha);
        if (u256_is_zero(dpow[j])) return false;
        win.zscale[j - 1] = f.inverse(dpow[j]);
        const size_t k = j - 1;                          // x_{k+1}: coordinate u^_k, history h_{k,i}
        for (size_t g = 0; g < n; ++g) win.Psi[k - 1][g] = f.mul(delta[j], win.X[j][g]);
        win.psi[k - 1] = f.mul(delta[j], win.X[j][G]);
        for (size_t i = 1; i < k; ++i)
            hist[(size_t)mfma_window_hist((int)k) + (i - 1)] = f.mul(f.mul(delta[j], win.X[j][n + i - 1]), win.zscale[i - 1]);
    }
    return true;
}

// the last history constant searched for a small multiple, and what was found (the constant depends on M and alpha only: one search per config)
struct SmallHistory {
    bool valid = false;
    U256 h1 = {{0, 0, 0, 0}}, lambda = {{0, 0, 0, 0}};
    uint32_t small = 0;
};

// The window's scales under delta_1 = 1 - or, for a window of three S-boxes whose history term is a table product (t = 3), under the
// delta_1 with h_{2,1} = 1 .. 4 where one exists; hist_small: that integer, or left as it is
inline bool window_choose_scale(const HostField &f, uint32_t t, uint32_t K, uint64_t alpha, Window &win, U256 *hist, SmallHistory &memo,
                                uint32_t &hist_small) {
    const U256 zero = {{0, 0, 0, 0}};
    win.lane0 = f.r;
    if (!window_scales(f, t, K, alpha, f.r, win, hist)) return false;
    if (!(alpha >= 2 && K == 3 && win.kw == 3 && mfma_hist_tab((int)t))) return true;
    const U256 h1 = hist[0];
    if (u256_is_zero(h1)) return true;
    if (!memo.valid || !u256_eq(memo.h1, h1)) {
        memo.valid = true;
        memo.h1 = h1;
        memo.small = 0;
        const U256 h1_inv = f.inverse(h1);
        U256 small = zero;
        for (uint32_t sm = 1; sm <= 4 && !memo.small; ++sm) {
            small = f.add(small, f.r);               // sm in the Montgomery domain
            if (host_root_window_scale(f, f.mul(small, h1_inv), alpha, memo.lambda)) memo.small = sm;
        }
    }
    if (!memo.small) return true;
    U256 small = zero;
    for (uint32_t i = 0; i < memo.small; ++i) small = f.add(small, f.r);
    if (window_scales(f, t, K, alpha, memo.lambda, win, hist) && u256_eq(hist[0], small)) {
        win.lane0 = memo.lambda;
        hist_small = memo.small;
        return true;
    }
    return window_scales(f, t, K, alpha, f.r, win, hist);
}

// the other coordinates: lanes of sigma themselves, chosen so that Psi stays invertible
inline bool window_complete_basis(const HostField &f, uint32_t t, Window &win) {
    const U256 zero = {{0, 0, 0, 0}};
    const size_t n = t - 1;
    size_t have = win.kw - 1, cand = 0;
    while (have < n) {
        if (cand >= n) return false;
        HostMat trial(win.Psi.begin(), win.Psi.begin() + (long)have);
        trial.push_back(std::vector<U256>(n, zero));
        trial.back()[cand] = f.r;
        if (mat_rank(f, trial) == have + 1) {
            win.Psi[have] = trial.back();
            ++have;
        }
        ++cand;
    }
    return mat_inverse(f, win.Psi, win.PsiInv);
}

// rows of a producing layer: P[i] = true lane i at the start of window `win` over the producer's inputs (n_in + 1 coefficients)
inline void window_emit(const HostField &f, uint32_t t, const std::vector<U256> &ark, const Window &win, const std::vector<Form> &P, size_t n_in,
                        std::vector<U256> &rows, std::vector<U256> &aff) {
    const U256 zero = {{0, 0, 0, 0}};
    const size_t n = t - 1;
    rows.assign((size_t)t * n_in, zero);
    aff.assign(t, zero);
    for (size_t g = 0; g < n_in; ++g) rows[g] = f.mul(win.lane0, P[0][g]);
    aff[0] = f.mul(win.lane0, f.add(P[0][n_in], ark[(size_t)win.first_round * t]));
    for (size_t k = 0; k < n; ++k) {
        for (size_t g = 0; g <= n_in; ++g) {
            U256 acc = zero;
            for (size_t l = 0; l < n; ++l) acc = f.add(acc, f.mul(win.Psi[k][l], P[1 + l][g]));
            if (g < n_in) rows[(1 + k) * n_in + g] = acc;
            else aff[1 + k] = f.add(acc, win.psi[k]);
        }
    }
}

inline bool derive_window_layers(const HostField &f, uint32_t t, uint32_t half, uint32_t rp, uint64_t alpha, uint32_t K,
                                 const std::vector<U256> &ark, const HostMat &M, const std::vector<U256> &entrance_scale,
                                 const std::vector<U256> &exit_scale, const U256 *arkopt_exit, WindowPlan &plan) {
    if (K < 1 || K > t || rp == 0 || half == 0 || entrance_scale.size() != t || exit_scale.size() != t) return false;
    const U256 zero = {{0, 0, 0, 0}};
    const size_t n = t - 1, G = n + K;
    const size_t n_win = (rp + K - 1) / K, nh = (size_t)mfma_window_hist((int)K);
    plan = WindowPlan();
    plan.n_win = n_win;
    plan.rows.resize(n_win);
    plan.aff.resize(n_win);
    plan.hist.assign(n_win * nh, zero);
    plan.hist_small.assign(n_win, 0u);
    std::vector<Window> wins(n_win);
    SmallHistory memo;
    uint32_t r1 = half;
    for (size_t w = 0; w < n_win; ++w) {
        Window &win = wins[w];
        win.kw = w == 0 ? rp - (uint32_t)(n_win - 1) * K : K;
        win.first_round = r1;
        r1 += win.kw;
        window_affine_forms(f, t, K, ark, M, win);
        if (!window_choose_scale(f, t, K, alpha, win, plan.hist.data() + w * nh, memo, plan.hist_small[w])) return false;
        if (!window_complete_basis(f, t, win)) return false;
    }
    {   // entry layer: inputs = scaled S-box outputs of the entrance round, true z_j = in_j / e_j, state = M z
        std::vector<Form> P(t, Form(t + 1, zero));
        for (size_t j = 0; j < t; ++j) {
            if (u256_is_zero(entrance_scale[j])) return false;
            const U256 inv = f.inverse(entrance_scale[j]);
            for (size_t i = 0; i < t; ++i) P[i][j] = f.mul(M[i][j], inv);
        }
        window_emit(f, t, ark, wins[0], P, t, plan.entry_rows, plan.entry_aff);
    }
    for (size_t w = 0; w < n_win; ++w) {
        const Window &win = wins[w];
        // the window's end state over its own inputs (u^, z^): sigma = PsiInv (u^ - psi), z_j = zscale_j z^_j
        std::vector<U256> shift = mat_vec(f, win.PsiInv, win.psi);   // PsiInv psi
        std::vector<Form> P(t, Form(G + 1, zero));
        for (size_t i = 0; i < t; ++i) {
            const Form &S = win.Send[i];
            for (size_t m = 0; m < n; ++m) {
                U256 acc = zero;
                for (size_t l = 0; l < n; ++l) acc = f.add(acc, f.mul(S[l], win.PsiInv[l][m]));
                P[i][m] = acc;
            }
            for (size_t j = 0; j < K; ++j) P[i][n + j] = f.mul(S[n + j], win.zscale[j]);   // (zero columns for the rounds a short window lacks)
            U256 cst = S[G];
            for (size_t l = 0; l < n; ++l) cst = f.sub(cst, f.mul(S[l], shift[l]));
            P[i][G] = cst;
        }
        if (w + 1 < n_win) {
            window_emit(f, t, ark, wins[w + 1], P, G, plan.rows[w], plan.aff[w]);
        } else {   // into the full rounds: D (s + c) - (the constant the kernel adds at that round)
            const size_t after = (size_t)(win.first_round + win.kw) * t;   // the first round after the section
            plan.rows[w].assign((size_t)t * G, zero);
            plan.aff[w].assign(t, zero);
            for (size_t i = 0; i < t; ++i) {
                for (size_t g = 0; g < G; ++g) plan.rows[w][i * G + g] = f.mul(exit_scale[i], P[i][g]);
                plan.aff[w][i] = f.sub(f.mul(exit_scale[i], f.add(P[i][G], ark[after + i])), arkopt_exit[i]);
            }
        }
    }
    return true;
}
}  // namespace pmx
