"""pmx_sponge_grind on the device against the oracle's C restatement (tests/grind_oracle.py: candidate states built on the host,
CRef.permute_batch, the canonical low bits by limbs_to_elems - never the library under test).

The rule: v is accepted iff  c = sponge.clone(); c.absorb(&F::from(v)); c.squeeze_bits(bits)  is all false (src/poseidon/mod.rs:232-254,
272-286); the entry returns the SMALLEST accepted nonce of [first, first + count) or "none".  Covered: every engine (named through
pmx_ctx_engine_info), smallest-not-any with many hits per wave and with the minimum in the last partial wave, the range edges around the
first hit, every mode at rate 2 and rate 8 (three of them through the shared pre-permutation) with the winner confirmed by check_pow
through the existing absorb / squeeze-bits entries, nonces across 2^32 and up to 2^64, a search that finds nothing, a search over several
chunks (chunk size set through the test library's hook), and the argument errors.  Seeds are fixed; where a case needs the oracle's hits
to have a shape (a hit at all, a gap of a wave, a hit in the third chunk) the test asserts that shape of the ORACLE before it asks the
product, so a changed seed fails loudly instead of testing nothing."""
import ctypes

import numpy as np
import pytest

import sponge_amd as S
from sponge_amd import _lib
from sponge_amd._lib import MODE_ABSORBING as A, MODE_SQUEEZING as Q

import grind_oracle as G

pytestmark = pytest.mark.gpu

ENGINE = {"quad": b"QuadEngine<5>", "window-t3": b"HybridEngine<3,5", "t9-bn254": b"HybridEngine<9,5", "lds-t16": b"LdsEngine<5>"}
# (label, engine, seed, count): the window engine of t = 3 starts above 32768 units; 40000 is the issue's cell
CELLS = [("t3", "quad", 0, 300), ("t3", "window-t3", 0, 40000), ("t9-bn254", "t9-bn254", 1, 300), ("lds-t16", "lds-t16", 0, 130)]


def grind(label, seed, tag, index, bits, first, count):
    f, cfg, _, _ = G.config(label)
    state = np.array(G.sponge_state(label, seed))
    before = state.tobytes()
    got = cfg.context(0).sponge_grind(state, tag, index, bits, first, count)
    assert state.tobytes() == before, "the caller's state was modified"
    return got


def engine_of(label, n):
    _, cfg, _, _ = G.config(label)
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(cfg.context(0)._h, _lib.OP_GRIND, n, 0, ctypes.byref(info)))
    return info.engine


@pytest.mark.parametrize("label,engine,seed,count", CELLS, ids=[c[1] for c in CELLS])
def test_every_engine_returns_the_oracles_first_hit(label, engine, seed, count):
    assert engine_of(label, count).startswith(ENGINE[engine]), engine_of(label, count)
    want = G.hits(label, seed, A, 0, 0, count, 6)
    assert want, "the seed gives the oracle no hit: the cell would test nothing"
    assert grind(label, seed, A, 0, 6, 0, count) == want[0]


@pytest.mark.parametrize("label,engine,seed,count", CELLS, ids=[c[1] for c in CELLS])
def test_smallest_not_any_with_hits_in_most_waves(label, engine, seed, count):
    """bits = 2: a quarter of the nonces is accepted - several hits per wave, hits in most waves, every workgroup of the launch racing for
    the result word; the minimum must come out, from ranges that start at different lanes and end in a partial wave"""
    wide = (0, count)
    ranges = [(0, count), (1, count - 1), (3, count - 5), (count // 2 + 5, count - count // 2 - 5)]
    assert any(cnt % 64 for _, cnt in ranges)
    for first, cnt in ranges:
        if engine == "window-t3" and cnt <= 32768:
            continue                                         # (would leave the engine under test)
        want = G.hits(label, seed, A, 0, first, cnt, 2, inside=wide)
        assert len(want) > cnt // 8
        assert grind(label, seed, A, 0, 2, first, cnt) == want[0], (first, cnt)


@pytest.mark.parametrize("label,seed,span,lanes", [("t9-bn254", 1, 600, 64), ("t3", 0, 300, 16), ("lds-t16", 0, 400, 64)],
                         ids=["t9-bn254", "quad", "lds-t16"])
def test_the_minimum_in_the_last_partial_wave(label, seed, span, lanes):
    """a range whose only hits lie in its LAST, partial wave (`lanes` units per wave: 64, or 16 quads on the quad engine): first is put
    right behind one oracle hit, so that the next one - at least a wave further on - is the minimum, and count ends a few units behind it
    inside the same wave.  bits = 6, where gaps of a wave exist."""
    all_hits = G.hits(label, seed, A, 0, 0, span, 6)
    pairs = [(a, b) for a, b in zip(all_hits, all_hits[1:]) if (b - a - 1) >= lanes and (b - a - 1) % lanes < lanes - 2]
    assert pairs, "no gap of a whole wave between two oracle hits: choose another seed"
    prev, h = pairs[0]
    first = prev + 1
    count = h - first + 2                                     # ends one unit behind the hit
    assert (h - first) // lanes == (count - 1) // lanes >= 1 and count % lanes != 0 and first + count <= span
    want = G.hits(label, seed, A, 0, first, count, 6, inside=(0, span))
    assert want and want[0] == h
    assert grind(label, seed, A, 0, 6, first, count) == h


# (the window engine's cell with a seed whose oracle hits leave a run of more than 32768 rejected nonces inside the 40000)
EDGE_CELLS = [c if c[1] != "window-t3" else (c[0], c[1], 16, c[3]) for c in CELLS]


@pytest.mark.parametrize("label,engine,seed,count", EDGE_CELLS, ids=[c[1] for c in EDGE_CELLS])
def test_range_edges_around_the_first_hit(label, engine, seed, count):
    """h = the oracle's first hit at or after first: a range that ends right in front of h finds nothing, one unit more finds h.  On the
    window engine of t = 3 both ranges must hold more than 32768 candidates: the difficulty and `first` are chosen, from the oracle's
    hits over the cell's range, so that h lies that far behind first."""
    edges = []
    for bits in ([6] if engine != "window-t3" else range(12, 18)):
        found = G.hits(label, seed, A, 0, 0, count, bits)
        for prev, h in zip([-1] + found, found):
            first = prev + 1 if engine == "window-t3" else prev + 2
            if h - first > (32768 if engine == "window-t3" else 0):
                edges.append((bits, first, h))
    assert edges, "the oracle's hits leave no such range: choose another seed"
    bits, first, h = edges[0]
    assert G.hits(label, seed, A, 0, first, h - first + 1, bits, inside=(0, count)) == [h]
    for n in (h - first, h - first + 1):
        assert engine_of(label, n).startswith(ENGINE[engine])
    assert grind(label, seed, A, 0, bits, first, h - first) is None
    assert grind(label, seed, A, 0, bits, first, h - first + 1) == h


MODES = [(A, 0), (A, 1), (A, "rate"), (Q, 0), (Q, "rate")]


@pytest.mark.parametrize("label,seed", [("t3", 2), ("t9-bn254", 2)], ids=["rate2", "rate8"])
@pytest.mark.parametrize("tag,index", MODES, ids=["absorbing0", "absorbing1", "absorbing_rate", "squeezing0", "squeezing_rate"])
def test_every_mode_and_the_winner_passes_check_pow(label, seed, tag, index):
    f, cfg, _, _ = G.config(label)
    index = cfg.rate if index == "rate" else index
    want = G.hits(label, seed, tag, index, 0, 300, 6)
    assert want, "the seed gives the oracle no hit in this mode"
    got = grind(label, seed, tag, index, 6, 0, 300)
    assert got == want[0]
    # the rule itself through the EXISTING absorb and squeeze-bits entries, on a copy of the sponge
    sponge = S.PoseidonSponge.from_state((np.array(G.sponge_state(label, seed)), S.DuplexSpongeMode(tag, index)), cfg)
    state_before, mode_before = sponge.state.tobytes(), sponge.mode
    assert sponge.grind(6, 0, 300) == got
    assert sponge.check_pow(got, 6)
    rejected = [v for v in range(got + 2) if v not in want][:3]
    assert rejected and not any(sponge.check_pow(v, 6) for v in rejected)
    assert sponge.state.tobytes() == state_before and sponge.mode == mode_before


@pytest.mark.parametrize("first", [(1 << 32) - 100, (1 << 64) - 300], ids=["across_2_32", "up_to_2_64"])
@pytest.mark.parametrize("label,seed", [("t3", 0), ("t9-bn254", 1)], ids=["quad", "t9-bn254"])
def test_wide_nonces(label, seed, first):
    """the residue of a nonce above 32 bits, and a range that ends exactly at 2^64 (first + count is never formed)"""
    want = G.hits(label, seed, A, 0, first, 300, 4)
    assert want and any(v >= 1 << 32 for v in want)
    assert grind(label, seed, A, 0, 4, first, 300) == want[0]
    later = [v for v in want if v >= (1 << 32)]
    assert grind(label, seed, A, 0, 4, later[0], first + 300 - later[0]) == later[0]
    if first + 300 == 1 << 64:
        assert grind(label, seed, A, 0, 4, first, None) == want[0]          # count None: up to 2^64
        last = want[-1]
        assert grind(label, seed, A, 0, 4, last, (1 << 64) - last) == last   # the last hit in front of 2^64, alone in its range


@pytest.mark.parametrize("label,seed", [("t3", 0), ("t9-bn254", 1)], ids=["quad", "t9-bn254"])
def test_none_found(label, seed):
    assert G.hits(label, seed, A, 0, 0, 1000, 60) == []
    f, cfg, _, _ = G.config(label)
    state = np.array(G.sponge_state(label, seed))
    before = state.tobytes()
    nonce, found = ctypes.c_uint64(0xABCD), ctypes.c_int(7)
    _lib.check(_lib.lib().pmx_sponge_grind(cfg.context(0)._h, ctypes.c_void_p(state.ctypes.data), A, 0, 60, 0, 1000, ctypes.byref(nonce),
                                           ctypes.byref(found)))
    assert found.value == 0 and nonce.value == 0xABCD
    assert state.tobytes() == before


def test_trivial_ranges_and_difficulties():
    assert grind("t3", 0, A, 0, 0, 12345, 10) == 12345        # bits = 0: every nonce is accepted
    assert grind("t3", 0, A, 0, 6, 12345, 0) is None          # count = 0
    assert grind("t3", 0, A, 0, 0, 12345, 0) is None
    assert grind("t3", 0, A, 0, 0, (1 << 64) - 1, 1) == (1 << 64) - 1


def _bind(handle, name):
    fn = getattr(handle, name)
    fn.restype, fn.argtypes = (_lib.SIGNATURES.get(name) or _lib.TEST_HOOK_SIGNATURES[name])
    return fn


@pytest.mark.parametrize("label,seed,bits,chunk", [("t3", 33, 9, 1000), ("t9-bn254", 32, 8, 200)], ids=["quad", "t9-bn254"])
def test_several_chunks(label, seed, bits, chunk):
    """the first hit in the THIRD chunk: two launches report nothing, the third one's minimum is the answer, and nothing behind it is
    searched.  The chunk size comes from the test library's hook (include/poseidon_mi355x_testing.h) - the product's chunk stays what it
    is, and the oracle leg stays three short chunks.  The test library is bound here next to whatever library the session uses."""
    count = 5 * chunk + 17
    want = G.hits(label, seed, A, 0, 0, count, bits)
    assert want and 2 * chunk <= want[0] < 3 * chunk, "the oracle's first hit is not in the third chunk: choose another seed"
    assert any(v >= 3 * chunk for v in want), "no later hit that a wrong walk could return"
    f, cfg, _, _ = G.config(label)
    hooks = ctypes.CDLL(_lib.TEST_LIB_PATH)
    create, destroy, grind_fn, set_chunk = (_bind(hooks, n) for n in ("pmx_ctx_create", "pmx_ctx_destroy", "pmx_sponge_grind", "pmx_test_grind_chunk"))
    c = S.poseidon.c_config(cfg)
    ctx = ctypes.c_void_p()
    assert create(ctypes.byref(c), 0, ctypes.byref(ctx)) == _lib.PMX_OK
    try:
        assert set_chunk(chunk) == _lib.PMX_OK
        state = np.array(G.sponge_state(label, seed))
        nonce, found = ctypes.c_uint64(0), ctypes.c_int(0)
        for first, cnt, expect in ((0, count, want[0]), (0, 2 * chunk + (want[0] - 2 * chunk), None), (7, count - 7, want[0])):
            found.value = 0
            assert grind_fn(ctx, ctypes.c_void_p(state.ctypes.data), A, 0, bits, first, cnt, ctypes.byref(nonce), ctypes.byref(found)) == _lib.PMX_OK
            assert (nonce.value if found.value else None) == expect, (first, cnt)
    finally:
        set_chunk(0)
        destroy(ctx)
    assert grind(label, seed, A, 0, bits, 0, count) == want[0]   # and the product's own chunk agrees


def test_errors_launch_nothing():
    lib = _lib.lib()
    for label, modulus_bits in (("t3", 255), ("t9-bn254", 254)):
        f, cfg, _, _ = G.config(label)
        h = cfg.context(0)._h
        state = np.array(G.sponge_state(label, 0))
        p = ctypes.c_void_p(state.ctypes.data)
        nonce, found = ctypes.c_uint64(0x5555), ctypes.c_int(9)
        n, fd = ctypes.byref(nonce), ctypes.byref(found)
        bad = [
            (h, p, A, 0, modulus_bits, 0, 10, n, fd, b"bits"),                       # bits = B: a second element would be needed
            (h, p, A, 0, 1 << 31, 0, 10, n, fd, b"bits"),
            (h, p, A, 0, 6, (1 << 64) - 299, 300, n, fd, b"2^64"),                  # first + count > 2^64
            (h, p, 2, 0, 6, 0, 10, n, fd, b"mode tag"),
            (h, p, A, cfg.rate + 1, 6, 0, 10, n, fd, b"mode index"),
            (h, p, Q, cfg.rate + 1, 6, 0, 10, n, fd, b"mode index"),
            (None, p, A, 0, 6, 0, 10, n, fd, b"null"),
            (h, None, A, 0, 6, 0, 10, n, fd, b"null"),
            (h, p, A, 0, 6, 0, 10, None, fd, b"null"),
            (h, p, A, 0, 6, 0, 10, n, None, b"null"),
        ]
        for *args, needle in bad:
            assert lib.pmx_sponge_grind(*args) == _lib.PMX_ERR_ARG, args
            assert needle in lib.pmx_last_error(), (needle, lib.pmx_last_error())
            assert nonce.value == 0x5555 and found.value == 9, "an error wrote a result"
        assert modulus_bits == f.modulus_bit_size
        # bits = B - 1 is the most one element yields: accepted (and, at that difficulty, nothing is found among 70 nonces)
        assert lib.pmx_sponge_grind(h, p, A, 0, modulus_bits - 1, 0, 70, n, fd) == _lib.PMX_OK and found.value == 0
        info = _lib.PmxEngineInfo()
        assert lib.pmx_ctx_engine_info(h, 6, 10, 0, ctypes.byref(info)) == _lib.PMX_ERR_ARG      # PMX_OP_GRIND is the last op
