"""The window engines of a modulus that is 1 mod 2^29 (BLS12-381 Fr: HybridEngineP1, S-boxes with complemented quotient digits -
sponge_amd/csrc/pmx_field.hpp) against the C restatement fed the oracle's constants, on batches with a one-lane tail wave and a one-lane
tail workgroup, and BN254 Fr - which keeps the generic step - next to them.

At t = 3 the dispatch hands calls of up to 32768 units to the quad engine, so every t = 3 shape runs twice: as stated (65, 257, 130 units -
whatever engine the dispatch picks) and 32768 units further up, where it is the window engine that meets the same tails."""
import ctypes

import numpy as np
import pytest

import sponge_amd as S
from sponge_amd import _lib, synth
from oracle import cref
from oracle import poseidon_oracle as O

from gpu_helpers import c_oracle, product_config
from helpers import oracle_config

pytestmark = pytest.mark.gpu

QUAD_MAX = 32768


def edge_states(f, p, t, first_ark, n, seed):
    """n states: all zero, all p - 1, all 1, one whose lane 0 cancels the first round constant (the first S-box input is 0), the rest random"""
    states = synth.random_elements(f, n * t, seed=seed).reshape(n, t, 4)
    states[0] = 0
    states[1] = f.from_ints([p - 1] * t)
    states[2] = f.from_ints([1] * t)
    states[3, 0] = f.from_ints([(p - first_ark) % p])[0]
    states[n - 1] = f.from_ints([p - 1] * t)          # the lone lane of the tail wave
    return states


def permute_dev(ctx, states):
    """pmx_permute_batch_dev on a buffer of the ABI's own allocator"""
    lib = _lib.lib()
    n = states.shape[0]
    d = ctypes.c_void_p()
    _lib.check(lib.pmx_device_alloc(0, ctypes.byref(d), states.nbytes))
    try:
        _lib.check(lib.pmx_device_upload(0, d, ctypes.c_void_p(states.ctypes.data), states.nbytes, None))
        ctx.permute_batch_dev(d.value, n, 0)
        back = np.zeros_like(states)
        _lib.check(lib.pmx_device_download(0, ctypes.c_void_p(back.ctypes.data), d, back.nbytes, None))
        _lib.check(lib.pmx_stream_synchronize(0, None))
    finally:
        _lib.check(lib.pmx_device_free(0, d))
    return back


def engine(ctx, op, n):
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(ctx._h, op, n, 0, ctypes.byref(info)))
    return info.engine


@pytest.mark.parametrize("n", [65, 257, QUAD_MAX + 65, QUAD_MAX + 257])
@pytest.mark.parametrize("name", ["bls_t3_a5_8_31", "bls_t3_a17_8_31"])
def test_t3_permutations_with_tail_lanes(name, n):
    cfg, cr, oc = product_config(name), c_oracle(name), oracle_config(name)
    ctx = cfg.context()
    if n > QUAD_MAX:
        assert engine(ctx, _lib.OP_PERMUTE, n).startswith(b"HybridEngine<3,"), engine(ctx, _lib.OP_PERMUTE, n)
    states = edge_states(cfg.field, oc.p, 3, oc.ark[0][0], n, 0x5EED0A00 + n)
    assert np.array_equal(permute_dev(ctx, states), cr.permute_batch(states, threads=0))


@pytest.mark.parametrize("rate", [3, 7])
def test_t4_and_t8_permutations_with_a_tail_lane(rate):
    """history rows on the matrix cores, three- and two-wave kernels"""
    f, p, t = S.BLS12_381_FR, O.BLS12_381_FR, rate + 1
    cfg = S.poseidon_config_from_lfsr(f, rate, 5, 8, 56 if rate == 3 else 57)
    oc = O.make_config(p, 255, rate, 5, 8, 56 if rate == 3 else 57)
    ctx = cfg.context()
    assert engine(ctx, _lib.OP_PERMUTE, 65).startswith(b"HybridEngine<%d,5" % t)
    states = edge_states(f, p, t, oc.ark[0][0], 65, 0x5EED0A10 + rate)
    assert np.array_equal(permute_dev(ctx, states), cref.CRef(oc).permute_batch(states, threads=0))


@pytest.mark.parametrize("n", [130, QUAD_MAX + 130])
def test_two_to_one_compressions(n):
    """one tree level of n compressions (a forest of n two-leaf trees): lane 0 enters as zero, lane 1 alone leaves"""
    name = "bls_t3_a5_8_31"
    cfg, cr, oc = product_config(name), c_oracle(name), oracle_config(name)
    ctx = cfg.context()
    if n > QUAD_MAX:
        assert engine(ctx, _lib.OP_COMPRESS, n).startswith(b"HybridEngine<3,5")
    pairs = edge_states(cfg.field, oc.p, 2, oc.ark[0][1], n, 0x5EED0A20 + n)
    nodes, roots = ctx.merkle_2to1_forest(pairs.reshape(n, 2, 4), n)
    assert np.array_equal(np.asarray(roots).reshape(n, 4), cr.hash_batch(pairs, 2, 1, threads=0).reshape(n, 4))


@pytest.mark.parametrize("n", [65, QUAD_MAX + 65])
def test_hash_rows(n):
    """rows of four elements to one (two permutations a row)"""
    name = "bls_t3_a5_8_31"
    cfg, cr, oc = product_config(name), c_oracle(name), oracle_config(name)
    ctx = cfg.context()
    if n > QUAD_MAX:
        assert engine(ctx, _lib.OP_HASH, n).startswith(b"HybridEngine<3,5")
    msgs = edge_states(cfg.field, oc.p, 4, oc.ark[0][1], n, 0x5EED0A30 + n)
    assert np.array_equal(ctx.hash_batch(msgs, 4, 1), cr.hash_batch(msgs, 4, 1, threads=0))


@pytest.mark.parametrize("n", [65, QUAD_MAX + 65])
def test_bn254_keeps_the_generic_step(n):
    """p = 1 mod 2^28 only: the same kernels as before serve it, on either side of the quad engine's range"""
    name = "bn254_t3_a5_8_57"
    cfg, cr, oc = product_config(name), c_oracle(name), oracle_config(name)
    assert oc.p % (1 << 29) != 1
    states = edge_states(cfg.field, oc.p, 3, oc.ark[0][0], n, 0x5EED0A40 + n)
    assert np.array_equal(permute_dev(cfg.context(), states), cr.permute_batch(states, threads=0))
