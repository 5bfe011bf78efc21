"""Edge values planted INSIDE the permutation, through its inverse (oracle/inverse.py), for tests/test_plants.py (CPU) and
tests/test_gpu_planted_edges.py.

A test that chooses the input reaches round 0 alone: from round 1 on every value the device sees is uniformly random, and the special
cases of the arithmetic - a lane that is exactly 0, 1, p - 1, a Montgomery image that is exactly 1, 2^29 - 1, 2^29, p - 1 - are met with
probability 2^-250.  Poseidon is a permutation, so a state chosen at any round boundary has an input; plants(name) returns those inputs.

Edge set E (canonical integers):  0, 1, 2, p - 1, (p - 1) / 2, and e * 2^-256, e * 2^-261 for e in {1, 2^29 - 1, 2^29, p - 1} - the
engines hold values scaled by 2^256 or 2^261, so these are the values whose stored words are e.

Plants, at EVERY round r = 0 .. R - 1 and at the output (nothing is thinned):
  sbox_in   every lane's S-box input (the state after ARK) is an edge, lane i takes E[(i + r + k) mod |E|]; one state per rotation k, so
            every lane meets every edge at every round
  lane0     partial rounds: lane 0's S-box input is each edge, the other lanes seeded random
  sbox_out  partial rounds: lane 0's S-box OUTPUT is each edge (its input is e^(1/alpha)), the other lanes seeded random
  output    one state per rotation with every output lane an edge, and one state per (lane, edge) with the other lanes seeded random

What keeps a wrong inverse from going unnoticed: the expected outputs are the C port's (oracle.cref, permute_batch), never the inverse
code's; for every plant the forward walk of the Python oracle (inverse.trace_many) must pass through the planted values at the planted
round; and C port and Python oracle must agree on every output.  A wrong inverse can only make a plant miss, loudly.

Nothing here opens a GPU or imports the library under test.  Results are cached per config for the session."""
import collections
import functools
import random
import time

import numpy as np

from oracle import cref
from oracle import inverse as I
from oracle import poseidon_oracle as O

from helpers import golden

# fuzz_configs.random_prime(255, top_byte=127) of tools/diag/fuzz_configs.py with rng = random.Random(0x127): the first draw that is
# prime and has gcd(5, p - 1) = 1.  Top byte 127: the int8 tables of the window engines store its larger residues as Y - p.
P127 = 0x7F73F68DDDC0883D1A17342355759A4DB5D1210C3D5395501A24003FF56ECE0F    # (tests/test_plants.py draws it again)
P127_SEED = 0x127

FIELDS = {"bls12_381_fr": (O.BLS12_381_FR, 255), "bn254_fr": (O.BN254_FR, 254)}
# beyond tests/golden/config_pins.json: name -> (modulus, prime bits, rate, alpha, RF, RP)
EXTRA_CONFIGS = {
    "bls_t16_a5_4_6": (O.BLS12_381_FR, 255, 15, 5, 4, 6),          # the run-time-width config of tests/grind_oracle.py ("lds-t16")
    "p127_t3_a5_8_31": (None, 255, 2, 5, 8, 31),                   # (modulus: P127)
}
# every config the planted-edge tests use
NAMES = ("bls_t3_a5_8_31", "bls_t3_a17_8_31", "bn254_t3_a5_8_57", "bls_t4_a5_8_56", "bls_t9_a5_8_57", "bn254_t9_a5_8_57",
         "bls_t16_a5_4_6", "p127_t3_a5_8_31")

Plant = collections.namedtuple("Plant", "kind round lane edge rotation")     # lane / edge / rotation: None where they do not apply
Plants = collections.namedtuple("Plants", "name cfg plants inputs expected seconds")


def draw_p127(seed=P127_SEED):
    """the draw the constant pins, by the algorithm of fuzz_configs.random_prime (Miller-Rabin on the same bases)"""
    rng = random.Random(seed)
    while True:
        c = rng.getrandbits(255) | (1 << 254) | 1
        c = (c & ((1 << 248) - 1)) | (127 << 248)
        if is_prime(c) and (c - 1) % 5:
            return c


def is_prime(n):
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for q in bases:
        if n % q == 0:
            return n == q
    d, r = n - 1, 0
    while d % 2 == 0:
        d //= 2
        r += 1
    for a in bases:
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


def parameters(name):
    """(modulus, prime bits, rate, alpha, RF, RP)"""
    if name in EXTRA_CONFIGS:
        p, bits, rate, alpha, rf, rp = EXTRA_CONFIGS[name]
        return (P127 if p is None else p), bits, rate, alpha, rf, rp
    d = golden("config_pins.json")[name]
    p, bits = FIELDS[d["field"]]
    return p, bits, d["rate"], d["alpha"], d["full_rounds"], d["partial_rounds"]


@functools.lru_cache(maxsize=None)
def oracle_config(name):
    p, bits, rate, alpha, rf, rp = parameters(name)
    return O.make_config(p, bits, rate, alpha, rf, rp)


@functools.lru_cache(maxsize=None)
def c_port(name):
    return cref.CRef(oracle_config(name))


def edges(p):
    """[(label, canonical integer)]"""
    out = [("0", 0), ("1", 1), ("2", 2), ("p-1", p - 1), ("(p-1)/2", (p - 1) // 2)]
    for shift in (256, 261):
        scale = pow(1 << shift, -1, p)
        for label, e in (("1", 1), ("2^29-1", 2**29 - 1), ("2^29", 2**29), ("p-1", p - 1)):
            out.append(("%s*2^-%d" % (label, shift), e * scale % p))
    return out


def partial_rounds(cfg):
    return [r for r in range(cfg.full_rounds + cfg.partial_rounds) if not I.is_full_round(cfg, r)]


def planted_states(cfg, seed):
    """[(Plant, r, the state at the start of round r before its ARK)] for every plant of the header"""
    p, t = cfg.p, cfg.t
    total = cfg.full_rounds + cfg.partial_rounds
    E = [v for _, v in edges(p)]
    rng = random.Random(seed)
    d = I.alpha_inverse(cfg)
    roots = I.powers(E, d, p, use_c=False)                    # e^(1/alpha)
    out = []

    def before_ark(r, after):
        return [(v - k) % p for v, k in zip(after, cfg.ark[r])]

    for r in range(total):
        for k in range(len(E)):
            out.append((Plant("sbox_in", r, None, None, k), r, before_ark(r, [E[(i + r + k) % len(E)] for i in range(t)])))
    for r in partial_rounds(cfg):
        for k, e in enumerate(E):
            out.append((Plant("lane0", r, 0, k, None), r, before_ark(r, [e] + [rng.randrange(p) for _ in range(t - 1)])))
        for k in range(len(E)):
            out.append((Plant("sbox_out", r, 0, k, None), r, before_ark(r, [roots[k]] + [rng.randrange(p) for _ in range(t - 1)])))
    for k in range(len(E)):
        out.append((Plant("output", total, None, None, k), total, [E[(i + k) % len(E)] for i in range(t)]))
    for lane in range(t):
        for k, e in enumerate(E):
            state = [rng.randrange(p) for _ in range(t)]
            state[lane] = e
            out.append((Plant("output", total, lane, k, None), total, state))
    return out


def expected_count(cfg):
    n_e, rp, total = len(edges(cfg.p)), cfg.partial_rounds, cfg.full_rounds + cfg.partial_rounds
    return n_e * (total + 2 * rp + 1 + cfg.t)


def check_hits(cfg, plants, sbox_in, sbox_out, out):
    """every plant's values are where they were planted, in the forward walk (sbox_in / sbox_out [R][t][n], out [t][n]); returns the
    indices of the plants that MISS"""
    E = [v for _, v in edges(cfg.p)]
    t = cfg.t
    missed = []
    for i, pl in enumerate(plants):
        if pl.kind == "sbox_in":
            ok = all(sbox_in[pl.round][lane][i] == E[(lane + pl.round + pl.rotation) % len(E)] for lane in range(t))
        elif pl.kind == "lane0":
            ok = sbox_in[pl.round][0][i] == E[pl.edge]
        elif pl.kind == "sbox_out":
            ok = sbox_out[pl.round][0][i] == E[pl.edge]
        elif pl.rotation is not None:
            ok = all(out[lane][i] == E[(lane + pl.rotation) % len(E)] for lane in range(t))
        else:
            ok = out[pl.lane][i] == E[pl.edge]
        if not ok:
            missed.append(i)
    return missed


@functools.lru_cache(maxsize=None)
def plants(name):
    """Plants(name, oracle config, [Plant], inputs [n][t][4] ABI limbs, the C port's outputs [n][t][4], seconds spent); read-only"""
    started = time.perf_counter()
    cfg = oracle_config(name)
    p, t = cfg.p, cfg.t
    states = planted_states(cfg, seed=0x9147 + NAMES.index(name))
    assert len(states) == expected_count(cfg)
    descr = [s[0] for s in states]
    xs = I.back_to_many(cfg, [(r, state) for _, r, state in states])
    sbox_in, sbox_out, out = I.trace_many(cfg, xs)
    missed = check_hits(cfg, descr, sbox_in, sbox_out, out)
    assert missed == [], ("plants the oracle's forward walk does not pass through", name, [descr[i] for i in missed[:5]])
    inputs = cref.elems_to_limbs([v for x in xs for v in x], p).reshape(len(xs), t, 4)
    expected = c_port(name).permute_batch(inputs, threads=0)
    oracle_out = cref.elems_to_limbs([int(out[lane][i]) for i in range(len(xs)) for lane in range(t)], p).reshape(len(xs), t, 4)
    assert np.array_equal(expected, oracle_out), ("C port and Python oracle differ on a planted input", name)
    inputs.setflags(write=False)
    expected.setflags(write=False)
    return Plants(name, cfg, tuple(descr), inputs, expected, time.perf_counter() - started)


def output_plants(pl):
    """indices of the plants of kind output"""
    return [i for i, d in enumerate(pl.plants) if d.kind == "output"]


def padded(pl, n, seed, last=None):
    """[n][t][4] ABI limbs: the planted inputs first, seeded random states behind them; `last`: the index of a plant that is ALSO
    the last unit (of a one-lane tail wave where n = 64 k + 1).  Returns (states, the C port's outputs)."""
    p, t = pl.cfg.p, pl.cfg.t
    k = pl.inputs.shape[0]
    assert n >= k + (last is not None)
    rng = random.Random(seed)
    fill = cref.elems_to_limbs([rng.randrange(p) for _ in range((n - k) * t)], p).reshape(n - k, t, 4)
    states = np.concatenate([pl.inputs, fill])
    if last is not None:
        states[n - 1] = pl.inputs[last]
    return states, c_port(pl.name).permute_batch(states, threads=0)


# ---- grind: sponges whose digest for one nonce has a chosen number of low zero bits -------------------------------------------------
GRIND_BITS = (28, 29, 30, 31, 32, 33, 57, 58, 63, 64, 65, 87, 128, 200, "B-2", "zero")
MODE_ABSORBING, MODE_SQUEEZING = 0, 1                      # DuplexSpongeMode tags (include/poseidon_mi355x.h, oracle.ABSORBING / SQUEEZING)


def grind_bits(name, b):
    """(b as a number, bits to ask for): "B-2" is prime bits - 2; "zero" is a digest of exactly 0, asked for at bits = B - 1"""
    bits = parameters(name)[1]
    if b == "B-2":
        return bits - 2, bits - 2
    if b == "zero":
        return None, bits - 1
    return b, b


@functools.lru_cache(maxsize=None)
def grind_case(name, b, squeezing, span):
    """(state [t][4] ABI limbs, tag, index, v, first, count, digest): a sponge that, for the nonce v of [first, first + span), squeezes
    the digest 2^b * odd (b a number) or 0 (b "zero").  Absorbing{1}: an output plant (digest lane = capacity) walked back, F::from(v)
    taken off lane capacity + 1.  squeezing: Squeezing{0} - the same for Absorbing{0}, walked back through one more permutation, the
    one such a sponge runs before it absorbs (mod.rs:250)."""
    cfg = oracle_config(name)
    p, t, cap = cfg.p, cfg.t, cfg.capacity
    total = cfg.full_rounds + cfg.partial_rounds
    number, _ = grind_bits(name, b)
    rng = random.Random("%s/%s/%d" % (name, b, squeezing))
    if number is None:
        digest = 0
    else:
        odd = rng.randrange(0, ((p - 1) >> number) + 1) | 1
        if odd << number >= p:
            odd -= 2
        digest = odd << number
        assert 0 < digest < p and digest % (1 << number) == 0 and (digest >> number) & 1
    out = [rng.randrange(p) for _ in range(t)]
    out[cap] = digest
    x = I.back_to(cfg, out, total)
    index = 0 if squeezing else 1
    v = rng.randrange(1 << 20, 1 << 40)
    first = v - rng.randrange(span // 4, span - span // 4)
    x[cap + index] = (x[cap + index] - v) % p
    if squeezing:
        x = I.back_to(cfg, x, total)
    state = cref.elems_to_limbs(x, p).reshape(t, 4)
    state.setflags(write=False)
    return state, (MODE_SQUEEZING if squeezing else MODE_ABSORBING), index, v, first, span, digest


def grind_digests(name, state, tag, index, first, count):
    """the acceptance rule from the C port alone (as tests/grind_oracle.py: digests): the canonical integer of the first squeezed element
    for every nonce of [first, first + count)"""
    cfg, cr = oracle_config(name), c_port(name)
    p = cfg.p
    base = np.array(state, dtype=np.uint64)
    if tag == MODE_SQUEEZING or index == cfg.rate:
        base = cr.permute_batch(base[None], threads=1)[0]
        index = 0
    at = cfg.capacity + index
    states = np.repeat(base[None], count, axis=0)
    lane = O.from_limbs([int(x) for x in base[at]])
    r = (1 << 256) % p
    states[:, at] = cref.elems_to_limbs([(lane + (first + k) * r) % p for k in range(count)], p, mont=False)   # += F::from(v)
    out = cr.permute_batch(states, threads=0)
    return cref.limbs_to_elems(out[:, cfg.capacity], p)


def first_hit(digests, first, bits):
    mask = (1 << bits) - 1
    return next((first + k for k, d in enumerate(digests) if d & mask == 0), None)
