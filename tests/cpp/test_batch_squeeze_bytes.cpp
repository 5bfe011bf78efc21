// BatchPoseidonSponge::squeeze_bytes / squeeze_bits of the C++ host mirror (sponge_amd/host/poseidon_sponge.hpp) - the device cut of
// pmx_sponge_squeeze_{bytes,bits}_batch - against the single PoseidonSponge of the same header, whose squeeze_bytes / squeeze_bits are
// host loops over squeeze_native_field_elements and fp_into_bigint (src/poseidon/mod.rs:256-286).  Needs a GPU.
#include <cstdio>
#include <string>

#include "../../sponge_amd/host/absorb.hpp"

using namespace pmx_host;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static void batch_equals_single_sponges(const Field &F, size_t rate) {
    auto param = get_default_poseidon_parameters(F, rate, false).value();
    const size_t n = 5;
    for (size_t num : {size_t(0), size_t(1), size_t(31), size_t(32), size_t(40), size_t(31 * rate + 1), size_t(254), size_t(255), size_t(600)}) {
        for (int bits = 0; bits < 2; ++bits) {
            auto batch = BatchPoseidonSponge::make(param, n);
            std::vector<Fp> in;
            for (uint64_t k = 0; k < n; ++k)
                for (uint64_t j = 0; j < 3; ++j) in.push_back(fp_from_u64(F, 100 * k + j));
            batch.absorb(in);
            (void)batch.squeeze_native_field_elements(1);   // Squeezing{1}: the cut starts inside the rate
            const std::vector<uint8_t> got = bits ? batch.squeeze_bits(num) : batch.squeeze_bytes(num);
            EXPECT(got.size() == n * num);
            for (uint64_t k = 0; k < n; ++k) {
                auto s = PoseidonSponge::make(param);
                s.absorb({in[3 * k], in[3 * k + 1], in[3 * k + 2]});
                (void)s.squeeze_native_field_elements(1);
                bool same = true;
                if (bits) {
                    const std::vector<bool> want = s.squeeze_bits(num);
                    for (size_t i = 0; i < num; ++i) same = same && got[k * num + i] == (want[i] ? 1 : 0);
                } else {
                    const std::vector<uint8_t> want = s.squeeze_bytes(num);
                    for (size_t i = 0; i < num; ++i) same = same && got[k * num + i] == want[i];
                }
                EXPECT(same);
                for (size_t i = 0; i < s.state.size(); ++i) EXPECT(s.state[i] == batch.state[k * s.state.size() + i]);
                EXPECT(batch.mode_tag[k] == (uint32_t)PMX_MODE_SQUEEZING && batch.mode_index[k] == s.mode.index);
            }
        }
    }
}

int main() {
    try {
        batch_equals_single_sponges(Field::bls12_381_fr(), 2);
        batch_equals_single_sponges(Field::bls12_381_fr(), 8);
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
