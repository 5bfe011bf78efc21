"""The acceptance rule of pmx_sponge_grind from the oracle's C restatement (oracle/cref), for tests/test_gpu_grind.py.  Nothing here calls
the product's device code: the candidates' states are built on the host with Python integers, CRef.permute_batch permutes them, and
limbs_to_elems gives the canonical integers whose low bits decide.

A nonce v is accepted iff  c = sponge.clone(); c.absorb(&F::from(v)); c.squeeze_bits(bits)  is all false (src/poseidon/mod.rs:232-254,
272-286): an Absorbing{rate} or Squeezing sponge permutes first (:239-252), then F::from(v) is added into state[capacity + index], the
squeeze permutes (:324-328) and hands out state[capacity] first; for bits below the modulus bit length its low bits are the answer."""
import functools

import numpy as np

import sponge_amd as S
from sponge_amd import synth
from sponge_amd._lib import MODE_ABSORBING, MODE_SQUEEZING
from oracle import cref
from oracle import poseidon_oracle as O

import merkle_ary_oracle as M

# label: (config of tests/merkle_ary_oracle.py, rate, capacity)
LABELS = {"t3": 2, "t9-bn254": 8, "lds-t16": 15}


def config(label):
    """(product field, product config, C port, modulus)"""
    f, cfg, cr = M.config(label)
    return f, cfg, cr, cr.cfg.p


@functools.lru_cache(maxsize=None)
def sponge_state(label, seed):
    """a mid-stream state [t][4] (every lane a seeded element, the capacity lane included); read-only"""
    f, cfg, _, _ = config(label)
    st = synth.random_elements(f, cfg.t, seed=0x6121D + seed).reshape(cfg.t, 4)
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def digests(label, seed, tag, index, first, count):
    """the canonical integer of the first squeezed element for every nonce of [first, first + count), in nonce order (a tuple)"""
    f, cfg, cr, p = config(label)
    base = np.array(sponge_state(label, seed))
    if tag == MODE_SQUEEZING or index == cfg.rate:                 # mod.rs:241-244, 250: the same permutation for every nonce
        base = cr.permute_batch(base[None], threads=1)[0]
        index = 0
    at = cfg.capacity + index
    states = np.repeat(base[None], count, axis=0)
    lane = O.from_limbs([int(x) for x in base[at]])                # the Montgomery residue as an integer
    r = (1 << 256) % p
    for k in range(count):
        states[k, at] = np.array(O.to_limbs((lane + (first + k) * r) % p), dtype=np.uint64)  # += F::from(v): residues add (mod.rs:128)
    out = cr.permute_batch(states, threads=0)
    return tuple(cref.limbs_to_elems(out[:, cfg.capacity], p))


def hits(label, seed, tag, index, first, count, bits, inside=None):
    """the accepted nonces of the range, ascending; `inside` = (first, count) of a cached wider range to cut the digests from"""
    wide_first, wide_count = inside or (first, count)
    assert wide_first <= first and first + count <= wide_first + wide_count
    d = digests(label, seed, tag, index, wide_first, wide_count)
    mask = (1 << bits) - 1
    return [first + k for k in range(count) if d[first - wide_first + k] & mask == 0]
