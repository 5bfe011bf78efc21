"""The row finish of the matrix-core layers on the device (sponge_amd/csrc/pmx_mfma.hpp: mfma_row_home) against the C restatement.

Rows of at most 15 inputs fold their byte sums in pairs on the lane that holds them and exchange eight registers with lane l +- 32
instead of sixteen, so a mistake in the exchange shows where a wave is not full: the batches are 64 states (one full wave), 65 (one lane
past it) and 193 (a last wave half empty).  At t = 3 the dispatch hands calls of up to 32768 units to the quad engine, which has no
matrix-core rows; every t = 3 shape therefore runs as stated AND 32768 units further up, where the window engine meets the same tails.

Inputs: seeded random states with all-zero states, states of p - 1 and states whose bytes are 0x7f / 0x80 patterns (reduced mod p:
bytes at both ends of the signed range of the matrix cores' operands) placed on both halves of a wave and on the tail lanes, and
batches made of such states alone."""
import ctypes

import numpy as np
import pytest

import sponge_amd as S
from sponge_amd import _lib, synth
from oracle import cref
from oracle import poseidon_oracle as O

pytestmark = pytest.mark.gpu

QUAD_MAX = 32768
SIZES = [64, 65, 193]

# field, oracle modulus, bits, t, partial rounds: what it exercises
CONFIGS = {
    "bls_t3": (S.BLS12_381_FR, O.BLS12_381_FR, 255, 3, 31),     # the P1 engine: short first window, free-scale history
    "bn254_t3": (S.BN254_FR, O.BN254_FR, 254, 3, 57),           # the generic step
    "bls_t4": (S.BLS12_381_FR, O.BLS12_381_FR, 255, 4, 56),     # history rows and operand-form rows
    "bls_t8": (S.BLS12_381_FR, O.BLS12_381_FR, 255, 8, 57),     # 15 inputs: the edge of the bound
    "bn254_t9": (S.BN254_FR, O.BN254_FR, 254, 9, 57),           # paired dense and history rows beside unpaired window rows in one kernel
}
_cache = {}


def config(key):
    if key not in _cache:
        f, p, bits, t, rp = CONFIGS[key]
        _cache[key] = (S.poseidon_config_from_lfsr(f, t - 1, 5, 8, rp), cref.CRef(O.make_config(p, bits, t - 1, 5, 8, rp)))
    return _cache[key]


def edge_elements(p):
    """0, p - 1 and the 0x7f / 0x80 byte patterns reduced mod p"""
    pats = [b"\x7f" * 32, b"\x80" * 32, b"\x7f\x80" * 16, b"\x80\x7f" * 16, b"\x80" * 16 + b"\x7f" * 16]
    return [0, p - 1] + [int.from_bytes(b, "little") % p for b in pats]


def mixed_states(f, p, t, n, seed):
    """random states; edge states on lanes 0 .. 6, 31 .. 37 (either side of the exchange) and the last lanes of the batch"""
    states = synth.random_elements(f, n * t, seed=seed).reshape(n, t, 4)
    edges = edge_elements(p)
    for base in (0, 31, n - len(edges)):
        for i, e in enumerate(edges):
            states[(base + i) % n] = f.from_ints([e] * t)
    states[(44) % n] = f.from_ints([edges[(2 + j) % len(edges)] for j in range(t)])     # patterns mixed inside one state
    return states


def edge_only_states(f, p, t, n):
    """no random state at all: blocks of eight equal edge states, so that lanes l and l + 32 hold different kinds"""
    edges = edge_elements(p)
    rows = [[edges[(i // 8) % len(edges)]] * t for i in range(n)]
    return f.from_ints([x for r in rows for x in r]).reshape(n, t, 4)


def permute_dev(ctx, states):
    """pmx_permute_batch_dev on a buffer of the ABI's own allocator"""
    lib = _lib.lib()
    d = ctypes.c_void_p()
    _lib.check(lib.pmx_device_alloc(0, ctypes.byref(d), states.nbytes))
    try:
        _lib.check(lib.pmx_device_upload(0, d, ctypes.c_void_p(states.ctypes.data), states.nbytes, None))
        ctx.permute_batch_dev(d.value, states.shape[0], 0)
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


def sizes_of(key):
    return SIZES + [QUAD_MAX + n for n in SIZES] if CONFIGS[key][3] == 3 else SIZES


CASES = [(key, n) for key in CONFIGS for n in sizes_of(key)]


@pytest.mark.parametrize("key,n", CASES, ids=["%s-%d" % c for c in CASES])
def test_permutations_bit_equal_on_full_and_partial_waves(key, n):
    f, p, bits, t, rp = CONFIGS[key]
    cfg, cr = config(key)
    ctx = cfg.context()
    if t > 3 or n > QUAD_MAX:
        assert engine(ctx, _lib.OP_PERMUTE, n).startswith(b"HybridEngine<%d,5" % t), engine(ctx, _lib.OP_PERMUTE, n)
    for what, states in (("random and edge states", mixed_states(f, p, t, n, 0x50F1 + 7 * n + t)), ("edge states only", edge_only_states(f, p, t, n))):
        got, want = permute_dev(ctx, states), cr.permute_batch(states, threads=0)
        bad = np.flatnonzero((got != want).any(axis=(1, 2)))
        assert bad.size == 0, (what, "states that differ:", bad[:16].tolist())


@pytest.mark.parametrize("n", [65, QUAD_MAX + 65])
def test_two_to_one_compressions_at_t3(n):
    """one tree level of n compressions: lane 0 enters as zero (lane0_zero), one lane leaves - through the same rows"""
    f, p, bits, t, rp = CONFIGS["bls_t3"]
    cfg, cr = config("bls_t3")
    ctx = cfg.context()
    if n > QUAD_MAX:
        assert engine(ctx, _lib.OP_COMPRESS, n).startswith(b"HybridEngine<3,5")
    pairs = mixed_states(f, p, 2, n, 0x50F2 + n)
    nodes, roots = ctx.merkle_2to1_forest(pairs.reshape(n, 2, 4), n)
    assert np.array_equal(np.asarray(roots).reshape(n, 4), cr.hash_batch(pairs, 2, 1, threads=0).reshape(n, 4))


@pytest.mark.parametrize("n", [65, QUAD_MAX + 65])
@pytest.mark.parametrize("in_len,out_len", [(4, 1), (3, 2)])
def test_hash_batch_dev_at_t3(n, in_len, out_len):
    """pmx_hash_batch_dev on device buffers: rows of in_len elements to out_len (want_lo / want_hi of the last permutation)"""
    f, p, bits, t, rp = CONFIGS["bls_t3"]
    cfg, cr = config("bls_t3")
    ctx = cfg.context()
    if n > QUAD_MAX:
        assert engine(ctx, _lib.OP_HASH, n).startswith(b"HybridEngine<3,5")
    msgs = mixed_states(f, p, in_len, n, 0x50F3 + n + in_len)
    lib = _lib.lib()
    out = np.zeros((n, out_len, 4), dtype=np.uint64)
    d_in, d_out = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.pmx_device_alloc(0, ctypes.byref(d_in), msgs.nbytes))
    try:
        _lib.check(lib.pmx_device_alloc(0, ctypes.byref(d_out), out.nbytes))
        try:
            _lib.check(lib.pmx_device_upload(0, d_in, ctypes.c_void_p(msgs.ctypes.data), msgs.nbytes, None))
            ctx.hash_batch_dev(d_in.value, in_len, d_out.value, out_len, n, 0)
            _lib.check(lib.pmx_device_download(0, ctypes.c_void_p(out.ctypes.data), d_out, out.nbytes, None))
            _lib.check(lib.pmx_stream_synchronize(0, None))
        finally:
            _lib.check(lib.pmx_device_free(0, d_out))
    finally:
        _lib.check(lib.pmx_device_free(0, d_in))
    assert np.array_equal(out.reshape(n, out_len, 4), np.asarray(cr.hash_batch(msgs, in_len, out_len, threads=0)).reshape(n, out_len, 4))
