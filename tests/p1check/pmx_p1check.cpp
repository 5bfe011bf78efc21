// CPU-side check of the Montgomery products with COMPLEMENTED quotient digits (sponge_amd/csrc/pmx_field.hpp: mont_sqr_p1 / mont_mul_p1,
// the window engines of a modulus that is 1 mod 2^29) - test infrastructure like tests/hostcheck, which it leaves as it is: the templates
// the HIP kernels instantiate, compiled for the host and exported for tests/test_p1_step.py.  Elements cross this interface as their nine
// raw 29-bit limbs, so that the test sees representatives, not residues.
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -I sponge_amd/csrc tests/p1check/pmx_p1check.cpp -o tests/p1check/libpmx_p1check.so
#include <cstdint>
#include <cstring>
#include <string>

#define PMX_HOSTCHECK 1
#include "pmx_prepare.hpp"

using namespace pmx;

void pmx::hostcheck_track(int, const Fe &, const FieldRt &) {}
// inputs of the matrix-core layers: each must be norm and below 2^256 (pmx_mfma.hpp: mfma_cut_element)
static unsigned long long g_layer_inputs = 0, g_layer_inputs_too_large = 0;
void pmx::hostcheck_below_2_256(const Fe &x) {
    ++g_layer_inputs;
    bool bad = (x.l[kN - 1] >> (256 - kW * (kN - 1))) != 0;
    for (int i = 0; i < kN; ++i) bad |= x.l[i] > kMask;
    if (bad) ++g_layer_inputs_too_large;
}
extern "C" void p1_layer_inputs(unsigned long long *seen, unsigned long long *too_large) {
    *seen = g_layer_inputs;
    *too_large = g_layer_inputs_too_large;
}

static int prepare_field(const uint64_t modulus[4], Prepared &pp) {
    pmx_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    std::memcpy(cfg.modulus, modulus, 32);
    cfg.full_rounds = 2; cfg.partial_rounds = 0; cfg.rate = 1; cfg.capacity = 0; cfg.alpha = 5;
    static const uint64_t zeros[8] = {0};
    cfg.ark = zeros; cfg.mds = zeros;
    std::string err;
    return prepare(&cfg, pp, err);
}

// what prepare() records for the modulus: 1 = the engines with the complemented digits serve it
extern "C" int p1_unit_low_limb(const uint64_t modulus[4]) {
    Prepared pp;
    const int rc = prepare_field(modulus, pp);
    return rc ? -rc : (pp.unit_low_limb ? 1 : 0);
}

static Fe load_fe(const uint32_t *l) { Fe x; std::memcpy(x.l, l, sizeof x.l); return x; }

// op: 0 mont_mul_p1(a, b)   1 / 2 / 3 mont_sqr_p1<kP1In / kP1Sq / kP1Out>(a)   10 mont_mul(a, b)   11 mont_sqr(a)
//     20 / 21 / 22 fe_sbox<0 / 5 / 17, true>(a)   30 / 31 / 32 fe_sbox<0 / 5 / 17, false>(a); b[0], b[1] = the exponent of the generic chain
// A modulus that is not 1 mod 2^29 is refused for every op below 10 and the 20s (PMX_ERR_UNSUPPORTED), as the launcher never routes one there.
extern "C" int p1_op(const uint64_t modulus[4], int op, size_t n, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    Prepared pp;
    int rc = prepare_field(modulus, pp);
    if (rc) return rc;
    const FieldRt &f = pp.f;
    const bool special = op < 10 || (op >= 20 && op < 30);
    if (special && !pp.unit_low_limb) return PMX_ERR_UNSUPPORTED;
    for (size_t i = 0; i < n; ++i) {   // n cases, nine limbs each
        const Fe x = load_fe(a + kN * i), y = load_fe(b + kN * i);
        const uint64_t alpha = (uint64_t)y.l[0] | ((uint64_t)y.l[1] << 32);
        Fe r;
        switch (op) {
            case 0: r = mont_mul_p1(x, y, f); break;
            case 1: r = mont_sqr_p1<kP1In>(x, f); break;
            case 2: r = mont_sqr_p1<kP1Sq>(x, f); break;
            case 3: r = mont_sqr_p1<kP1Out>(x, f); break;
            case 10: r = mont_mul(x, y, f); break;
            case 11: r = mont_sqr(x, f); break;
            case 20: r = fe_sbox<0, true>(x, alpha, pp.one, f); break;
            case 21: r = fe_sbox<5, true>(x, 5, pp.one, f); break;
            case 22: r = fe_sbox<17, true>(x, 17, pp.one, f); break;
            case 30: r = fe_sbox<0, false>(x, alpha, pp.one, f); break;
            case 31: r = fe_sbox<5, false>(x, 5, pp.one, f); break;
            case 32: r = fe_sbox<17, false>(x, 17, pp.one, f); break;
            default: return PMX_ERR_ARG;
        }
        std::memcpy(out + kN * i, r.l, sizeof r.l);
    }
    return PMX_OK;
}

template <int T>
struct HostScratch {
    Fe slot[T - 1];
    Fe get(uint32_t i) const { return slot[i]; }
    void set(uint32_t i, const Fe &x) { slot[i] = x; }
};

static Abi load_abi(const uint64_t *p) { Abi a; std::memcpy(a.w, p, 32); return a; }
static void store_abi(uint64_t *p, const Abi &a) { std::memcpy(p, a.w, 32); }

// permute_hybrid as HybridEngineP1<T, alpha> instantiates it (P1 = true), the matrix-core layers as integer sums (pmx_mfma.hpp, host form)
template <int T>
static int permute_p1_t(const Prepared &pp, uint64_t *states, size_t n) {
    const OptTables tb = pp.opt_tables();
    constexpr int KW = mfma_window_for(T);
    if ((int)pp.mfma_window != KW) return PMX_ERR_UNSUPPORTED;
    for (size_t k = 0; k < n; ++k) {
        Fe s[T];
        HostScratch<T> sc;
        for (int i = 0; i < T; ++i) s[i] = fe_from_abi_scaled(load_abi(states + (k * T + i) * 4));
        const uint64_t *lane0 = states + (k * T) * 4;
        const bool z0 = !(lane0[0] | lane0[1] | lane0[2] | lane0[3]);
        if (pp.c.alpha == 5) permute_hybrid<T, 5, HostScratch<T>, KW, true>(s, sc, tb, pp.c, pp.one, pp.f, 0, T, z0);
        else permute_hybrid<T, 0, HostScratch<T>, KW, true>(s, sc, tb, pp.c, pp.one, pp.f, 0, T, z0);
        for (int i = 0; i < T; ++i) store_abi(states + (k * T + i) * 4, fe_to_abi_scaled(s[i], pp.f));
    }
    return PMX_OK;
}
extern "C" int p1_permute_hybrid(const pmx_config *cfg, uint64_t *states, size_t n) {
    Prepared pp;
    std::string err;
    int rc = prepare(cfg, pp, err);
    if (rc) return rc;
    if (!pp.has_opt || !pp.mfma_dense || !pp.unit_low_limb) return PMX_ERR_UNSUPPORTED;
    switch (pp.t) {
        case 3: return permute_p1_t<3>(pp, states, n);
        case 4: return permute_p1_t<4>(pp, states, n);
        case 5: return permute_p1_t<5>(pp, states, n);
        case 9: return permute_p1_t<9>(pp, states, n);
        default: return PMX_ERR_UNSUPPORTED;
    }
}
