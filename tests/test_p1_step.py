"""Montgomery products with COMPLEMENTED quotient digits (sponge_amd/csrc/pmx_field.hpp: mont_sqr_p1 / mont_mul_p1 - the S-boxes of the
window engines when the modulus is 1 mod 2^29, BLS12-381 Fr among them), on the host build of the very templates the kernels instantiate
(tests/p1check), against Python integers, the generic step and the oracle.

Stated for every form:  result * 2^261 = V + M p  with 0 <= M <= 2^261, i.e. the result is congruent to V 2^-261 and at most V / 2^261 + p
(mont_step's bound); kP1Out returns every limb below 2^29, kP1In / kP1Sq limb 0 in [1, 2^29] and the others below 2^29."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from sponge_amd._lib import PmxConfig
from oracle import cref
from oracle import poseidon_oracle as O

from helpers import golden, ints, oracle_config

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "p1check")
W, N = 29, 9
MASK = (1 << W) - 1
R = 1 << (W * N)

# primes that are 1 mod 2^29 besides BLS12-381 Fr: 255 bits with top byte 127 (residues above 127 S: pmx_prepare.hpp), 254 bits, 231 bits
P127 = 0x7FE25EA8BD7912EFEE60F553B2B761E3748A7D8348CBC9AB8D8E5A91E0000001
P254 = 0x28F9DE6C1F2CCE07AA9DD0675A2046D7EBCE6DA903E5BE203D38DEEAE0000001
P231 = 0x6DB090CA17DB5562CD083DEA1755BC1B9A53F93356C87CB60960000001
PRIMES = [O.BLS12_381_FR, P127, P254, P231]

MUL, SQR_IN, SQR_SQ, SQR_OUT, GEN_MUL, GEN_SQR = 0, 1, 2, 3, 10, 11
SBOX = {0: 20, 5: 21, 17: 22}
GEN_SBOX = {0: 30, 5: 31, 17: 32}


@pytest.fixture(scope="module")
def p1():
    subprocess.check_call(["make", "-C", HERE, "all"], stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(HERE, "libpmx_p1check.so"))
    lib.p1_op.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.p1_unit_low_limb.argtypes = [ctypes.c_void_p]
    lib.p1_permute_hybrid.argtypes = [ctypes.POINTER(PmxConfig), ctypes.c_void_p, ctypes.c_size_t]
    lib.p1_layer_inputs.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return lib


def limbs(x):
    assert 0 <= x < (1 << (W * (N - 1) + 32))
    return [(x >> (W * i)) & MASK for i in range(N - 1)] + [x >> (W * (N - 1))]


def value(l):
    return sum(int(v) << (W * i) for i, v in enumerate(l))


def modulus_words(p):
    return np.array(O.to_limbs(p), dtype=np.uint64)


def run(p1, p, op, a_cases, b_cases=None, expect=0):
    """a_cases / b_cases: lists of nine-limb lists; returns the results as lists of nine limbs"""
    a = np.array(a_cases, dtype=np.uint32).reshape(-1, N)
    b = np.array(b_cases if b_cases is not None else a_cases, dtype=np.uint32).reshape(-1, N)
    out = np.zeros_like(a)
    mod = modulus_words(p)
    rc = p1.p1_op(mod.ctypes.data, op, len(a), a.ctypes.data, b.ctypes.data, out.ctypes.data)
    assert rc == expect, rc
    return [[int(v) for v in row] for row in out]


def lazy(p, rng=None):
    """limbs at 2^30 - 1 (or random below 2^30) with a magnitude of at most 4 p: what fe_add_lazy hands an S-box"""
    top = (4 * p) >> (W * (N - 1))
    if rng is None:
        return [(1 << 30) - 1] * (N - 1) + [max(top - 1, 0)]
    return [rng.randrange(1 << 30) for _ in range(N - 1)] + [rng.randrange(max(top, 1))]


def as_near_norm(v):
    """v >= 1 as the squarings hand it on: limb 0 in [1, 2^29] (a zero limb 0 borrows 2^29 from above)"""
    l = limbs(v)
    if l[0] == 0:
        l = limbs(v - MASK - 1)
        l[0] += MASK + 1
    return l


def sqrt_mod_pow2(a, k):
    """x with x^2 = a mod 2^k (a = 1 mod 8)"""
    x = 1
    for bit in range(3, k):
        if (x * x - a) % (1 << (bit + 1)):
            x += 1 << (bit - 1)
    assert (x * x - a) % (1 << k) == 0
    return x


def check_form(r, v_seen, p, out_form):
    """r 2^261 = V + M p with 0 <= M <= 2^261, and the limb ranges of the form"""
    diff = value(r) * R - v_seen
    assert diff % p == 0 and 0 <= diff // p <= R, (r, diff // p if diff % p == 0 else None)
    assert all(l <= MASK for l in r[1:N - 1])
    if out_form:
        assert r[0] <= MASK
    else:
        assert 1 <= r[0] <= MASK + 1


def mul_cases(p, rng, n_random):
    """(a, b): a norm or nearly so (what the S-box multiplies: x^(alpha-1)), b up to lazy (x)"""
    edge = [limbs(0), limbs(1), limbs(p - 1), [MASK] * N, lazy(p), limbs(int(7.59 * p)),
            limbs(1 << W), limbs(3 << (5 * W)), [0] + [MASK] * (N - 1), [1 << 15] + [5] * (N - 1), [1 << 14] + [7] * (N - 1)]
    pairs = [(a, b) for a in edge for b in edge]
    pairs += [(limbs(1 << (5 * W)), limbs(1 << (4 * W)))]              # V = 2^261: every low column is 0 (every digit all ones)
    for _ in range(4):                                               # V = -p mod 2^261: every low column comes out all ones (every digit 0)
        a = rng.randrange(p) | 1
        pairs.append((limbs(a), limbs(-p * pow(a, -1, R) % R)))
        pairs.append((limbs(a), limbs(-pow(a, -1, R) % R)))           # V = -1 mod 2^261
    pairs += [(limbs(rng.randrange(p)), limbs(rng.randrange(p))) for _ in range(n_random // 2)]
    pairs += [(limbs(rng.randrange(2 * p)), lazy(p, rng)) for _ in range(n_random - n_random // 2)]
    return pairs


def sqr_cases(p, rng, n_random, near_norm):
    """near_norm: operands of kP1Sq - limb 0 in [1, 2^29], the others below 2^29, below 2 p"""
    if near_norm:
        edge = [limbs(1), as_near_norm(p - 1), as_near_norm(p), as_near_norm(1 << 131), [MASK + 1] + [MASK] * (N - 2) + [(2 * p) >> (W * (N - 1))], [MASK + 1] + [0] * (N - 1),
                limbs(sqrt_mod_pow2(p, W * N)),                        # a^2 = p mod 2^261: V - 1 + N p = 0 takes every digit all ones
                limbs((1 << (W * 5)) + 1), [1] + [MASK] * (N - 1)]
        rnd = [limbs(rng.randrange(2 * p) | 1) for _ in range(n_random)]
        rnd += [[rng.randrange(1, MASK + 2)] + limbs(rng.randrange(p))[1:] for _ in range(n_random // 4)]
        return edge + rnd
    edge = [limbs(0), limbs(1), limbs(p - 1), [MASK] * N, lazy(p), limbs(int(7.59 * p)), limbs(1 << W), limbs(1 << 131),   # (2^131)^2 = 0 mod 2^261
            [0] + [MASK] * (N - 1), [1 << 15] + [3] * (N - 1)]
    return edge + [limbs(rng.randrange(4 * p)) for _ in range(n_random // 2)] + [lazy(p, rng) for _ in range(n_random - n_random // 2)]


@pytest.mark.parametrize("p", PRIMES)
def test_special_products_match_integers_and_generic_step(p1, p):
    assert p % (1 << W) == 1 and pow(2, p - 1, p) == 1
    rng = random.Random(p & 0xFFFFFF)
    pairs = mul_cases(p, rng, 10000)
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    got, gen = run(p1, p, MUL, a, b), run(p1, p, GEN_MUL, a, b)
    for x, y, r, g in zip(a, b, got, gen):
        check_form(r, value(x) * value(y), p, True)
        assert (value(r) - value(g)) % p == 0
    for op, near, out_form in [(SQR_IN, False, False), (SQR_OUT, False, True), (SQR_SQ, True, False)]:
        a = sqr_cases(p, rng, 10000, near)
        got, gen = run(p1, p, op, a), run(p1, p, GEN_SQR, a)
        for x, r, g in zip(a, got, gen):
            check_form(r, value(x) ** 2, p, out_form)
            assert (value(r) - value(g)) % p == 0


@pytest.mark.parametrize("p", PRIMES)
@pytest.mark.parametrize("alpha", [5, 17, 3, 0, 1, 2, 7, 257, (1 << 63) + 1])
def test_sbox_chain_matches_generic_and_stays_below_1_3_p(p1, p, alpha):
    """x^alpha through the special products: congruent to the generic chain's, normalised, and below 1.3 p for alpha >= 4 on every input an S-box
    can meet - lazy sums up to 4 p, the window S-box's normalised 7.6 p (pmx_field.hpp: fe_sbox states 1.3; the layers cut it into 32 bytes)"""
    rng = random.Random(alpha * 1000003 + (p & 0xFFFF))
    xs = [limbs(0), limbs(1), limbs(p - 1), limbs(p), lazy(p), limbs(int(7.59 * p)), limbs(1 << W), limbs(1 << 131), [0] + [MASK] * (N - 2) + [1]]
    xs += [limbs(rng.randrange(4 * p)) for _ in range(300)] + [lazy(p, rng) for _ in range(300)]
    kind = alpha if alpha in (5, 17) else 0
    e = [[alpha & 0xFFFFFFFF, alpha >> 32] + [0] * (N - 2)] * len(xs)
    got, gen = run(p1, p, SBOX[kind], xs, e), run(p1, p, GEN_SBOX[kind], xs, e)
    rinv = pow(R, -1, p)
    for x, r, g in zip(xs, got, gen):
        assert (value(r) - value(g)) % p == 0
        # x = X 2^261: x^alpha in the same form is X^alpha 2^261
        assert value(r) % p == pow(value(x) * rinv, alpha, p) * R % p
        assert all(l <= MASK for l in r[:N - 1])
        if alpha >= 4:
            assert value(r) * 10 < 13 * p
        assert value(r) < (1 << 256)


def replay_columns(form, a_max, b_max, p_max, sqr):
    """the schedule of mont_mul_p1 / mont_sqr_p1 with every operand limb, every modulus limb and every digit at its maximum: the largest value
    each column accumulator can hold (a_max, b_max: nine limb maxima; digits: 2^29 - 1, m_0 = 2^29 where the form counts it one up)"""
    acc, worst = 0, 0
    m = [MASK] * N
    if form != SQR_SQ:
        m[0] = MASK + 1
    for k in range(2 * N - 1):
        for i in range(N):
            j = k - i
            if not 0 <= j < N:
                continue
            if not sqr:
                acc += a_max[i] * b_max[j]
            elif j > i:
                acc += a_max[i] * 2 * a_max[j]
            elif j == i:
                acc += a_max[i] * a_max[i]
        for j in range(N):
            if (j < k if k < N else j >= k - (N - 1)) and 0 < k - j < N:
                acc += m[j] * p_max[k - j]
        if k == N - 1 and form in (MUL, SQR_OUT):
            acc += 1 << W
        worst = max(worst, acc)
        acc >>= W
    return worst, acc


def test_no_column_accumulator_leaves_64_bits():
    """Worst-case replay for every call site of permute_hybrid with the special products (fe_sbox<5 | 17 | 0, true>): the first squaring takes a
    lazily added x (limbs below 2^30, magnitude <= 4 p: top limb below 2^25) or the window's normalised 7.6 p; the later squarings a value
    with limb 0 <= 2^29; the closing product that value and x.  The accumulators are unsigned and the carries logical shifts: 64 bits."""
    p_max = [1] + [MASK] * (N - 2) + [(1 << (255 - W * (N - 1))) - 1]       # p < 2^255, p_0 = 1
    lazy_x = [(1 << 30) - 1] * (N - 1) + [(1 << 25) - 1]
    norm_x = [MASK] * (N - 1) + [(1 << 26) - 1]                              # 7.6 p < 2^258
    near = [MASK + 1] + [MASK] * (N - 2) + [(1 << 24) - 1]                   # a product: below 2 p < 2^256
    for form, a, b, sqr in [(SQR_IN, lazy_x, None, True), (SQR_IN, norm_x, None, True), (SQR_OUT, lazy_x, None, True),
                            (SQR_SQ, near, None, True), (SQR_OUT, near, None, True),
                            (MUL, near, lazy_x, False), (MUL, near, norm_x, False), (MUL, lazy_x, near, False)]:
        worst, top = replay_columns(form, a, b, p_max, sqr)
        assert worst < (1 << 64) and top < (1 << 32), (form, worst.bit_length())
    # the replay does find an overflow where there is one: squaring an operand with limbs up to 2^31
    worst, _ = replay_columns(SQR_IN, [(1 << 31) - 1] * N, None, p_max, True)
    assert worst >= (1 << 64)


def pmx_config(cfg):
    p = cfg.p
    ark = cref.elems_to_limbs([v for row in cfg.ark for v in row], p)
    mds = cref.elems_to_limbs([v for row in cfg.mds for v in row], p)
    c = PmxConfig()
    c.full_rounds, c.partial_rounds, c.alpha = cfg.full_rounds, cfg.partial_rounds, cfg.alpha
    c.rate, c.capacity = cfg.rate, cfg.capacity
    for i, l in enumerate(O.to_limbs(p)):
        c.modulus[i] = l
    c.ark, c.mds = ark.ctypes.data, mds.ctypes.data
    return c, (ark, mds)


def layer_inputs(p1):
    seen, bad = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    p1.p1_layer_inputs(ctypes.byref(seen), ctypes.byref(bad))
    return seen.value, bad.value


@pytest.mark.parametrize("name", ["bls_t3_a5_8_31", "bls_t3_a17_8_31", "bls_t4_a5_8_56", "bls_t9_a5_8_57", "bls_t3_a257_8_13"])
def test_permutation_with_special_products_matches_golden(p1, name):
    """permute_hybrid as HybridEngineP1 instantiates it, on the oracle's vectors: c2's config, alpha = 17, a generic exponent, t = 4 and t = 9;
    every input of every matrix-core layer normalised and below 2^256"""
    cfg = oracle_config(name)
    vecs = golden("permute_vectors.json")[name]
    states = cref.elems_to_limbs([x for v in vecs for x in ints(v["in"])], cfg.p).reshape(len(vecs), cfg.t, 4)
    want = [x for v in vecs for x in ints(v["out"])]
    c, keep = pmx_config(cfg)
    out = np.ascontiguousarray(states, dtype=np.uint64).copy()
    seen0, bad0 = layer_inputs(p1)
    assert p1.p1_permute_hybrid(ctypes.byref(c), out.ctypes.data, len(vecs)) == 0
    assert cref.limbs_to_elems(out, cfg.p) == want
    seen, bad = layer_inputs(p1)
    assert seen > seen0 and bad == bad0


@pytest.mark.parametrize("p,bits", [(P127, 255), (P231, 231)])
def test_permutation_of_another_prime_matches_oracle(p1, p, bits):
    rng = random.Random(bits)
    cfg = O.make_config(p, bits, 2, 5, 8, 31)
    states = [[0, 0, 0], [p - 1] * 3, [1, 1, 1], [0, rng.randrange(p), rng.randrange(p)]] + [[rng.randrange(p) for _ in range(3)] for _ in range(4)]
    want = [x for st in states for x in O.permute(cfg, st)]
    c, keep = pmx_config(cfg)
    out = cref.elems_to_limbs([x for st in states for x in st], p).reshape(len(states), 3, 4).copy()
    assert p1.p1_permute_hybrid(ctypes.byref(c), out.ctypes.data, len(states)) == 0
    assert cref.limbs_to_elems(out, p) == want


def test_other_moduli_are_never_routed_to_the_special_products(p1):
    """prepare() records the property (p mod 2^29 == 1) and nothing else reaches the special forms: BN254 Fr (2-adicity 28) and 2^255 - 19 keep the
    generic step"""
    for p, want in [(O.BLS12_381_FR, 1), (P127, 1), (P254, 1), (P231, 1), (O.BN254_FR, 0), ((1 << 255) - 19, 0)]:
        assert (p % (1 << W) == 1) == bool(want)
        assert p1.p1_unit_low_limb(modulus_words(p).ctypes.data) == want
    x = [limbs(5)]
    refused = p1.p1_op(modulus_words(O.BN254_FR).ctypes.data, 99, 1, np.zeros(N, dtype=np.uint32).ctypes.data,
                       np.zeros(N, dtype=np.uint32).ctypes.data, np.zeros(N, dtype=np.uint32).ctypes.data)
    assert refused != 0
    for op in (MUL, SQR_IN, SQR_SQ, SQR_OUT, SBOX[5], SBOX[17], SBOX[0]):
        a = np.array(x, dtype=np.uint32)
        out = np.zeros_like(a)
        rc = p1.p1_op(modulus_words(O.BN254_FR).ctypes.data, op, 1, a.ctypes.data, a.ctypes.data, out.ctypes.data)
        assert rc != 0 and not out.any(), (op, rc)
    assert run(p1, O.BN254_FR, GEN_MUL, x, x)   # the generic products serve it
    c, keep = pmx_config(oracle_config("bn254_t3_a5_8_57"))
    st = np.zeros((1, 3, 4), dtype=np.uint64)
    assert p1.p1_permute_hybrid(ctypes.byref(c), st.ctypes.data, 1) != 0


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
@pytest.mark.parametrize("t,alpha,max_vgprs,waves", [(3, 5, 128, 4), (3, 0, 128, 4), (9, 5, 256, 2)])
def test_special_permute_kernel_keeps_its_occupancy_without_scratch(t, alpha, max_vgprs, waves):
    """the budgets tests/test_kernel_resources.py pins for HybridEngine, for the kernels of a modulus that is 1 mod 2^29"""
    csrc = os.path.join(os.path.dirname(HERE), "..", "sponge_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "asm1", f"T={t}", f"ALPHA={alpha}", "EXTRA=-DPMX_ONE_P1"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rpt = open(os.path.join(csrc, "build", f"one_t{t}.rpt")).read()
    assert f"HybridEngineP1ILi{t}ELi{alpha}EEE" in rpt
    get = lambda key: int(re.search(key + r": (\d+)", rpt).group(1))
    assert get(r"ScratchSize \[bytes/lane\]") == 0, rpt[-1500:]
    assert get("VGPRs") + get("AGPRs") <= max_vgprs and get(r"Occupancy \[waves/SIMD\]") >= waves, rpt[-1500:]
