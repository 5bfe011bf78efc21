#!/usr/bin/env python3
"""Writes the configuration file tools/prepare_dump.cpp reads: every class of configuration the host tests and the fuzzer build, a seeded
random sweep, and the refusals of prepare() one by one.  Nothing here needs the library or a GPU: constants come from the oracle's Grain
LFSR (the named and directed configurations) or from a seeded generator (the sweep: random round constants, a Cauchy matrix).

One configuration per line:  name modulus rate capacity alpha full_rounds partial_rounds  then the round constants and the matrix, row-major,
as ABI Montgomery residues (x * 2^256 mod p), all numbers but the name in hex.
usage: tools/prepare_configs.py OUT [seed]     prints the number of configurations and the index of each group's first one"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import poseidon_oracle as O  # noqa: E402

BLS, BN = O.BLS12_381_FR, O.BN254_FR
PALLAS_FP = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001
P25519 = (1 << 255) - 19
SMALL_P = (1 << 230) + 0x1D                      # the pseudo-modulus of tests/test_hostcheck.py (field operations only)
P127 = 0x7FE25EA8BD7912EFEE60F553B2B761E3748A7D8348CBC9AB8D8E5A91E0000001      # the primes of tests/test_p1_step.py: 1 mod 2^29
P254 = 0x28F9DE6C1F2CCE07AA9DD0675A2046D7EBCE6DA903E5BE203D38DEEAE0000001
P231 = 0x6DB090CA17DB5562CD083DEA1755BC1B9A53F93356C87CB60960000001
P250 = 0x2ca0806c3cccc1b9c01d4041d309b8d3b3806aefb11c60086a765dae8b3ccc5
ALPHAS = [0, 1, 1, 2, 3, 4, 5, 5, 5, 6, 7, 11, 17, 17, 257, 65537, (1 << 32) + 1, (1 << 63) + 1, (1 << 64) - 1]   # tools/diag/fuzz_configs.py


def is_prime(n):
    for q in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % q == 0:
            return n == q
    d, r = n - 1, 0
    while d % 2 == 0:
        d //= 2
        r += 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def random_prime(rng, bits, top_byte=None):
    while True:
        c = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        if top_byte is not None:
            c = (c & ((1 << 248) - 1)) | (top_byte << 248)
        if is_prime(c):
            return c


class Writer:
    def __init__(self, path):
        self.f = open(path, "w")
        self.n = 0
        self.groups = []

    def group(self, name):
        self.groups.append((name, self.n))

    def raw(self, name, modulus, rate, capacity, alpha, rf, rp, ark, mds):
        """ark, mds: flat lists of the words prepare() is handed (no conversion)"""
        self.f.write(" ".join([name.replace(" ", "_")] + ["%x" % v for v in [modulus, rate, capacity, alpha, rf, rp] + list(ark) + list(mds)]) + "\n")
        self.n += 1

    def config(self, name, cfg, rate=None, capacity=None):
        """an oracle config (canonical integers); rate / capacity: another split of the same width"""
        p = cfg.p
        mont = lambda v: (v << 256) % p
        rate, capacity = (cfg.rate, cfg.capacity) if rate is None else (rate, capacity)
        assert rate + capacity == cfg.t
        self.raw(name, p, rate, capacity, cfg.alpha, cfg.full_rounds, cfg.partial_rounds, [mont(v) for row in cfg.ark for v in row],
                 [mont(v) for row in cfg.mds for v in row])

    def lfsr(self, name, p, t, alpha, rf, rp, capacity=1):
        self.config(name, O.make_config(p, p.bit_length(), t - 1, alpha, rf, rp), t - capacity, capacity)

    def seeded(self, name, rng, p, t, alpha, rf, rp, capacity):
        """random round constants and a Cauchy matrix 1 / (x_i + y_j)"""
        while True:
            xs, ys = [rng.randrange(p) for _ in range(t)], [rng.randrange(p) for _ in range(t)]
            if all((x + y) % p for x in xs for y in ys):
                break
        ark = [[rng.randrange(p) for _ in range(t)] for _ in range(rf + rp)]
        mds = [[pow((x + y) % p, -1, p) for y in ys] for x in xs]
        self.config(name, O.PoseidonConfig(p, rf, rp, alpha, ark, mds, t - capacity, capacity))


def main():
    out = sys.argv[1]
    rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 2024)
    w = Writer(out)
    golden = os.path.join(ROOT, "tests", "golden")

    w.group("tests/golden")
    for name, d in json.load(open(os.path.join(golden, "config_pins.json"))).items():
        p = {"bls12_381_fr": BLS, "bn254_fr": BN}[d["field"]]
        w.lfsr(name, p, d["rate"] + 1, d["alpha"], d["full_rounds"], d["partial_rounds"])
    d = json.load(open(os.path.join(golden, "reference_test_config.json")))
    w.config("reference_test_a17_8_29", O.PoseidonConfig(BLS, d["full_rounds"], d["partial_rounds"], d["alpha"], [[int(x, 16) for x in r] for r in d["ark"]],
                                                         [[int(x, 16) for x in r] for r in d["mds"]], d["rate"], d["capacity"]))

    w.group("fields")
    p225 = random_prime(rng, 225)
    fields = [("bls", BLS), ("bn254", BN), ("p25519", P25519), ("pallas", PALLAS_FP), ("p127", P127), ("p254", P254), ("p231", P231), ("p250", P250),
              ("p225", p225), ("p225b", random_prime(rng, 225)), ("p226", random_prime(rng, 226))]
    for fname, p in fields + [("small_p", SMALL_P)]:            # what the field-operation exports prepare: 2 + 0 rounds, width 1, zero constants
        w.raw("field_only_" + fname, p, 1, 0, 5, 2, 0, [0, 0], [0])
    for fname, p in fields:
        w.lfsr("%s_t3_8_31" % fname, p, 3, 5, 8, 31)
        w.lfsr("%s_t3_8_22" % fname, p, 3, 5, 8, 22)
        w.lfsr("%s_t9_8_22" % fname, p, 9, 5, 8, 22)
    for fname, p in [("bls", BLS), ("bn254", BN), ("p25519", P25519), ("p127", P127)]:
        w.lfsr("%s_t3_8_56" % fname, p, 3, 5, 8, 56)
        w.lfsr("%s_t9_8_57" % fname, p, 9, 5, 8, 57)
        w.lfsr("%s_t5_8_56" % fname, p, 5, 5, 8, 56)

    w.group("exponents")
    for alpha in (0, 1, 2, 3, 5, 17, 257, (1 << 63) + 1):
        for t, rp in ((3, 31), (5, 24), (9, 13)):
            w.lfsr("bls_t%d_a%x_8_%d" % (t, alpha, rp), BLS, t, alpha, 8, rp)
        w.lfsr("p25519_t3_a%x_8_13" % alpha, P25519, 3, alpha, 8, 13)

    w.group("round counts")
    for t in (2, 3, 4, 9, 12):
        for rf, rp in ((7, 22), (3, 5), (1, 4), (0, 6), (2, 1), (8, 0), (7, 0), (2, 0), (1, 0), (8, 1), (8, 2), (8, 3), (8, 4)):
            w.lfsr("bls_t%d_%d_%d" % (t, rf, rp), BLS, t, 5, rf, rp)
    # a partial section long enough to leave the optimised schedule (2^261 / p is about 70 for BLS12-381 Fr, 169 for BN254 Fr)
    for t in (3, 9):
        for fname, p, rp in (("bls", BLS, 66), ("bls", BLS, 67), ("bls", BLS, 70), ("bls", BLS, 200), ("bn254", BN, 160), ("bn254", BN, 180), ("p25519", P25519, 70)):
            w.lfsr("%s_t%d_8_%d" % (fname, t, rp), p, t, 5, 8, rp)
    for alpha in (2, 3):
        w.lfsr("bls_t3_a%d_8_66" % alpha, BLS, 3, alpha, 8, 66)

    w.group("widths")
    for t in range(2, 17):
        w.lfsr("bls_t%d_8_24" % t, BLS, t, 5, 8, 24)
        w.lfsr("bn254_t%d_a17_6_13_cap" % t, BN, t, 17, 6, 13, capacity=min(2, t - 1))
    w.lfsr("bls_t3_cap0", BLS, 3, 5, 8, 31, capacity=0)
    w.lfsr("bls_t3_cap2", BLS, 3, 5, 8, 31, capacity=2)

    w.group("directed shapes of tools/diag/fuzz_configs.py")
    directed = [("p127", 3, 1, 5, 8, 31), ("p127", 3, 1, 17, 8, 31), ("p127", 3, 1, 3, 8, 31), ("p127", 3, 1, 7, 8, 31), ("p127", 3, 1, 257, 8, 13),
                ("bls", 3, 1, 5, 8, 31), ("bls", 3, 1, 17, 8, 31), ("bn254", 3, 1, 5, 8, 57), ("bls", 3, 1, 5, 8, 0), ("bls", 3, 0, 5, 8, 31),
                ("p127", 5, 1, 5, 8, 56), ("p127", 9, 1, 17, 8, 57), ("p127", 7, 2, 5, 7, 22), ("bn254", 9, 1, 5, 8, 57), ("bls", 2, 1, 5, 8, 56),
                ("bn254", 12, 1, 5, 8, 57), ("bls", 6, 1, 5, 8, 0)]
    for fname, t, capacity, alpha, rf, rp in directed:
        p = {"bls": BLS, "bn254": BN}.get(fname) or random_prime(rng, 255, top_byte=127)
        w.lfsr("directed_%s_t%d_c%d_a%d_%d_%d" % (fname, t, capacity, alpha, rf, rp), p, t, alpha, rf, rp, capacity=capacity)

    w.group("seeded sweep")
    for k in range(240):
        if k % 4 == 3:
            p = random_prime(rng, 255, top_byte=127) if (k // 4) % 2 == 0 else random_prime(rng, rng.choice([225, 226, 233, 240, 247, 248, 249, 253, 254, 255]))
        elif k % 4 == 2:
            p = rng.choice([P25519, P127, P254, P231, PALLAS_FP])
        else:
            p = rng.choice([BLS, BN])
        t = rng.choice([2, 3, 3, 3, 4, 5, 6, 7, 8, 9, 9, 10, 11, 12, 13, 14, 15, 16])
        capacity = min(rng.choice([1, 1, 1, 0, 2, 3]), t - 1)
        alpha = rng.choice(ALPHAS)
        rf = rng.choice([0, 1, 2, 3, 4, 6, 7, 8, 8, 8, 10])
        rp = rng.choice([0, 1, 2, 3, 5, 6, 7, 13, 22, 31, 56, 57, 60, 66, 67, 70])
        if rf + rp == 0:
            rf = 2
        w.seeded("sweep%03d_%dbit_t%d_c%d_a%x_%d_%d" % (k, p.bit_length(), t, capacity, alpha, rf, rp), rng, p, t, alpha, rf, rp, capacity)

    w.group("refusals")
    base = O.make_config(BLS, 255, 2, 5, 8, 31)
    ark, mds = [(v << 256) % BLS for row in base.ark for v in row], [(v << 256) % BLS for row in base.mds for v in row]
    w.raw("refuse_even_modulus", BLS - 1, 2, 1, 5, 8, 31, ark, mds)
    w.raw("refuse_256_bit_modulus", (1 << 255) + 95, 2, 1, 5, 8, 31, ark, mds)
    w.raw("refuse_224_bit_modulus", (1 << 223) + 0x1B, 2, 1, 5, 8, 31, [v >> 40 for v in ark], [v >> 40 for v in mds])
    w.raw("refuse_width_17", BLS, 16, 1, 5, 2, 1, [1] * (3 * 17), [1] * (17 * 17))
    w.raw("refuse_zero_rounds", BLS, 2, 1, 5, 0, 0, [], mds)
    w.raw("refuse_4097_rounds", BLS, 2, 1, 5, 8, 4089, [1] * (4097 * 3), mds)
    w.raw("refuse_unreduced_ark", BLS, 2, 1, 5, 8, 31, ark[:40] + [BLS] + ark[41:], mds)
    w.raw("refuse_unreduced_mds", BLS, 2, 1, 5, 8, 31, ark, mds[:4] + [(1 << 256) - 1] + mds[5:])
    w.raw("refuse_rate_0", BLS, 0, 3, 5, 8, 31, ark, mds)
    w.f.close()
    print("%d configurations" % w.n)
    for name, first in w.groups:
        print("  %4d  %s" % (first, name))


if __name__ == "__main__":
    main()
