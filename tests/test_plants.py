"""The plant generator (tests/plants.py) and the inverse walk (oracle/inverse.py) on the CPU: round trips and trace hits for every
config the GPU test uses, the refusal of an S-box that is no bijection, the pinned prime, the grind sponges, and the SENSITIVITY check -
two subtly wrong forward walks that agree with the oracle on a seeded random batch of the same size and differ from it on a plant."""
import math
import random

import numpy as np
import pytest

from oracle import cref
from oracle import inverse as I
from oracle import poseidon_oracle as O

import plants as P


@pytest.mark.parametrize("name", P.NAMES)
def test_every_alpha_and_matrix_is_invertible(name):
    cfg = P.oracle_config(name)
    p, t = cfg.p, cfg.t
    assert math.gcd(cfg.alpha, p - 1) == 1
    d = I.alpha_inverse(cfg)
    for x in (0, 1, 2, p - 1, 0x1234567 * 2**200 % p):
        assert pow(pow(x, cfg.alpha, p), d, p) == x
    minv = I.mds_inverse(cfg)
    product = [[sum(cfg.mds[i][k] * minv[k][j] for k in range(t)) % p for j in range(t)] for i in range(t)]
    assert product == [[int(i == j) for j in range(t)] for i in range(t)]


def test_the_roots_in_c_equal_pow():
    p = O.BLS12_381_FR
    rng = random.Random(7)
    xs = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, 2**29, 2**64 - 1, 2**64, 2**128] + [rng.randrange(p) for _ in range(200)]
    for q in (p, O.BN254_FR, P.P127):
        for e in (0, 1, 5, pow(5, -1, q - 1), q - 2, (1 << 255) + 12345):
            want = [pow(x % q, e, q) for x in xs]
            assert I.powers([x % q for x in xs], e, q, use_c=False) == want
            assert I.powers([x % q for x in xs], e, q) == want        # (pow() again where no compiler is found)


@pytest.mark.parametrize("name", P.NAMES)
def test_round_trips(name):
    """back_to of a random state at every round boundary: the oracle's own permute gives the output back, and trace passes through it"""
    cfg = P.oracle_config(name)
    p, t, total = cfg.p, cfg.t, cfg.full_rounds + cfg.partial_rounds
    rng = random.Random(name)
    state = [rng.randrange(p) for _ in range(t)]
    assert O.permute(cfg, I.back_to(cfg, state, total)) == state
    assert I.back_to(cfg, state, 0) == state
    planted = [(r, [rng.randrange(p) for _ in range(t)]) for r in range(total + 1)]
    xs = I.back_to_many(cfg, planted)
    sbox_in, sbox_out, out = I.trace_many(cfg, xs)
    for k, (r, want) in enumerate(planted):
        if r < total:
            assert [(int(sbox_in[r][i][k]) - cfg.ark[r][i]) % p for i in range(t)] == want, r
        else:
            assert [int(v) for v in out[:, k]] == want
    for k in (0, total // 2, total):                                   # the batch walk is the single walk, and trace is permute
        assert I.back_to(cfg, planted[k][1], planted[k][0]) == xs[k]
        a, b, o = I.trace(cfg, xs[k])
        assert o == O.permute(cfg, xs[k]) == [int(v) for v in out[:, k]]
        for r in range(total):
            full = I.is_full_round(cfg, r)
            assert b[r] == [pow(v, cfg.alpha, p) if full or i == 0 else v for i, v in enumerate(a[r])]


@pytest.mark.parametrize("name", P.NAMES)
def test_every_plant_is_hit(name):
    """plants() asserts the hits and the agreement of C port and Python oracle itself; here: the counts, that nothing is thinned, and that
    the check can fail"""
    pl = P.plants(name)
    cfg = pl.cfg
    total, n_e = cfg.full_rounds + cfg.partial_rounds, len(P.edges(cfg.p))
    print("%-20s %5d plants  %.2f s" % (name, len(pl.plants), pl.seconds))
    assert n_e == 13 and len({v for _, v in P.edges(cfg.p)}) == 13
    assert len(pl.plants) == pl.inputs.shape[0] == P.expected_count(cfg)
    kinds = {}
    for d in pl.plants:
        kinds.setdefault(d.kind, set()).add((d.round, d.lane, d.edge, d.rotation))
    assert kinds["sbox_in"] == {(r, None, None, k) for r in range(total) for k in range(n_e)}
    assert kinds["lane0"] == kinds["sbox_out"] == {(r, 0, k, None) for r in P.partial_rounds(cfg) for k in range(n_e)}
    assert kinds["output"] == ({(total, None, None, k) for k in range(n_e)}
                               | {(total, lane, k, None) for lane in range(cfg.t) for k in range(n_e)})
    assert len(P.partial_rounds(cfg)) == cfg.partial_rounds
    # every lane meets every edge at every round
    for r in (0, total - 1):
        for lane in range(cfg.t):
            assert {(lane + r + k) % n_e for k in range(n_e)} == set(range(n_e))
    # a plant that is NOT there is reported: shift every description by one round
    xs = [cref.limbs_to_elems(x, cfg.p) for x in pl.inputs[:2 * n_e]]
    a, b, o = I.trace_many(cfg, xs)
    assert P.check_hits(cfg, pl.plants[:2 * n_e], a, b, o) == []
    shifted = [d._replace(round=d.round + 1) for d in pl.plants[:2 * n_e]]
    assert len(P.check_hits(cfg, shifted, a, b, o)) == 2 * n_e


def test_an_sbox_that_is_no_bijection_is_refused():
    p = O.BLS12_381_FR
    assert (p - 1) % 3 == 0
    cfg = O.make_config(p, 255, 2, 3, 8, 31)
    with pytest.raises(ValueError, match="gcd"):
        I.alpha_inverse(cfg)
    with pytest.raises(ValueError, match="gcd"):
        I.back_to(cfg, [1, 2, 3], 5)


def test_the_pinned_prime():
    assert P.P127 == P.draw_p127(P.P127_SEED)
    assert P.is_prime(P.P127) and P.P127.bit_length() == 255 and P.P127 >> 248 == 127
    assert math.gcd(5, P.P127 - 1) == 1 and P.P127 % 2**29 != 1


# ---- sensitivity: what the plants see and random data cannot -------------------------------------------------------------------------
def walk(cfg, x, final=lambda v, p: v % p, zero_round=None):
    """the round loop of O.permute with two places to be wrong in: the final reduction, and an S-box input of 0 in one partial round"""
    p, t, alpha = cfg.p, cfg.t, cfg.alpha
    s = list(x)
    for rnd in range(cfg.full_rounds + cfg.partial_rounds):
        s = [(s[i] + cfg.ark[rnd][i]) % p for i in range(t)]
        if I.is_full_round(cfg, rnd):
            s = [pow(v, alpha, p) for v in s]
        elif rnd == zero_round and s[0] == 0:
            s[0] = 1                                                     # (a kernel that took "the integer p" for a unit, say)
        else:
            s[0] = pow(s[0], alpha, p)
        s = [sum(cfg.mds[i][j] * s[j] for j in range(t)) for i in range(t)]
        s = [v % p for v in s] if rnd + 1 < cfg.full_rounds + cfg.partial_rounds else [final(v, p) for v in s]
    return s


def p_for_zero(v, p):
    """one conditional subtraction too few: p comes out where 0 should"""
    return v % p or p


@pytest.mark.parametrize("mutant", ["p_for_0_from_the_final_reduction", "sbox_input_0_in_partial_round_17"])
def test_mutants_pass_random_batches_and_fail_a_plant(mutant):
    name = "bls_t3_a5_8_31"
    pl = P.plants(name)
    cfg, p = pl.cfg, pl.cfg.p
    kwargs = {"final": p_for_zero} if mutant.startswith("p_for_0") else {"zero_round": 17}
    assert not I.is_full_round(cfg, 17)
    from sponge_amd import synth
    import sponge_amd as S
    n = len(pl.plants)
    batch = synth.random_elements(S.BLS12_381_FR, n * cfg.t, seed=0x5EED).reshape(n, cfg.t, 4)      # the seed of smoke()'s batch
    randoms = [cref.limbs_to_elems(x, p) for x in batch]
    planted = [cref.limbs_to_elems(x, p) for x in pl.inputs]
    assert walk(cfg, planted[0]) == O.permute(cfg, planted[0])                                     # the unmutated walk is the oracle
    assert all(walk(cfg, x, **kwargs) == O.permute(cfg, x) for x in randoms), "the mutant is caught by random data already"
    caught = [i for i, x in enumerate(planted) if walk(cfg, x, **kwargs) != O.permute(cfg, x)]
    assert caught, "no plant tells the mutant from the oracle"
    kinds = {pl.plants[i].kind for i in caught}
    print(mutant, "caught by", len(caught), "plants of kinds", sorted(kinds))
    assert kinds <= ({"output"} if mutant.startswith("p_for_0") else {"sbox_in", "lane0", "sbox_out"})


# ---- grind sponges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("squeezing", [False, True], ids=["absorbing1", "squeezing0"])
@pytest.mark.parametrize("name", ["bls_t3_a5_8_31", "bn254_t9_a5_8_57", "bls_t16_a5_4_6"])
def test_grind_sponges_have_the_digest_they_claim(name, squeezing):
    """for every b: the C port's digest for the nonce v is exactly 2^b * odd (or 0), so v is accepted at bits = b and not at b + 1"""
    bits_of_p = P.parameters(name)[1]
    for b in P.GRIND_BITS:
        state, tag, index, v, first, count, digest = P.grind_case(name, b, squeezing, 300)
        assert first <= v < first + count
        number, ask = P.grind_bits(name, b)
        got = P.grind_digests(name, state, tag, index, v, 1)[0]
        assert got == digest, (name, b)
        if number is None:
            assert got == 0 and ask == bits_of_p - 1
        else:
            assert got % (1 << number) == 0 and (got >> number) & 1 and ask == number
            assert P.first_hit([got], v, number) == v and P.first_hit([got], v, number + 1) is None
    assert P.grind_bits(name, "B-2")[0] == bits_of_p - 2
