// CPU-side check of the PAIRED ROW FINISH of the matrix-core layers (sponge_amd/csrc/pmx_mfma.hpp: mfma_pair_sums,
// mfma_row_acc_pairs_p) for tests/test_row_finish_pairs.py: everything pmx_hostcheck.cpp exports - the same templates, in one
// translation unit - plus the guard on the pairs of byte sums and the row finish one row at a time.  Test infrastructure only.
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -I sponge_amd/csrc tests/hostcheck/pmx_row_finish_check.cpp -o tests/hostcheck/libpmx_row_finish_check.so
#include "pmx_hostcheck.cpp"

// pairs of byte sums of the paired row finish (pmx_mfma.hpp: mfma_pair_sums): each must fit a signed 32-bit register, |Q| < 2^31 -
// counted on every pair of every row this build computes, the way hostcheck_below_2_256 guards the operand cut
static unsigned long long g_row_pairs = 0, g_row_pairs_too_large = 0;
void pmx::hostcheck_pair_fits_32(long long q) {
    ++g_row_pairs;
    if (q >= (1ll << 31) || q <= -(1ll << 31)) ++g_row_pairs_too_large;
}
extern "C" void hc_row_pairs(unsigned long long *seen, unsigned long long *too_large) {
    *seen = g_row_pairs;
    *too_large = g_row_pairs_too_large;
}

// The row finish one row at a time: 32 sums S_e, the row's eight correction words and a modulus in, the nine words a[] of V + m p out -
// from the paired form (mfma_row_acc_pairs_p over mfma_pair_sums) and from the four-weight form (mfma_row_acc_p) - and the row
// (V + m p) / 2^24 as nine 29-bit limbs, read out of the paired form's words.
extern "C" int hc_row_finish(const uint64_t modulus[4], const int32_t sums[32], const long long corr[8], uint32_t a_pairs[9], uint32_t a_four[9],
                             uint32_t limbs[9]) {
    pmx_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    std::memcpy(cfg.modulus, modulus, 32);
    cfg.full_rounds = 2; cfg.partial_rounds = 0; cfg.rate = 1; cfg.capacity = 0; cfg.alpha = 5;
    uint64_t zeros[8] = {0};
    cfg.ark = zeros; cfg.mds = zeros;
    Prepared pp;
    std::string err;
    int rc = prepare(&cfg, pp, err);
    if (rc) return rc;
    int32_t R[8][4], Q[8][2];
    for (int e = 0; e < 32; ++e) R[e / 4][e % 4] = sums[e];
    for (int w = 0; w < 8; ++w) Q[w][0] = mfma_pair_sums(R[w][0], R[w][1]), Q[w][1] = mfma_pair_sums(R[w][2], R[w][3]);
    uint32_t ap[9], af[9];
    mfma_row_acc_pairs_p(Q, corr, pp.f.io + kIoP32, pp.f.pinv, ap);
    mfma_row_acc_p(R, corr, pp.f.io + kIoP32, pp.f.pinv, af);
    const Fe row = mfma_row_limbs(ap);
    for (int i = 0; i < 9; ++i) a_pairs[i] = ap[i], a_four[i] = af[i], limbs[i] = row.l[i];
    return PMX_OK;
}
// which finish a row of n_in inputs takes (1: pairs), asked through the templates' own dispatch (mfma_row_acc_for) for the input counts
// listed: -1 where the form taken and the predicate disagree
template <int NIN>
static int row_form_of() {
    int32_t R[8][4] = {{0}};
    R[0][0] = 1; R[0][1] = 1;
    long long corr[8] = {0};
    const uint32_t p32[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    uint32_t a[9];
    const unsigned long long before = g_row_pairs;
    mfma_row_acc_for<NIN>(R, corr, p32, 0u, a);
    const bool took_pairs = g_row_pairs != before;
    return took_pairs == mfma_row_pairs(NIN) ? (took_pairs ? 1 : 0) : -1;
}
extern "C" int hc_row_form(int n_in) {
    switch (n_in) {
        case 3: return row_form_of<3>();
        case 5: return row_form_of<5>();
        case 9: return row_form_of<9>();
        case 15: return row_form_of<15>();
        case 16: return row_form_of<16>();
        case 17: return row_form_of<17>();
        default: return mfma_row_pairs(n_in) ? 1 : 0;
    }
}
