"""Edge values planted inside the permutation (tests/plants.py: through the inverse walk of oracle/inverse.py) on the device, bit for bit
against the oracle's C restatement.

Every parity test so far chooses inputs, and so reaches round 0 alone; from round 1 on the kernels have only ever seen uniformly random
values.  Here every engine instantiation below permutes inputs whose S-box inputs, S-box outputs and output lanes are exactly 0, 1, 2,
p - 1, (p - 1) / 2 or a value whose stored word (scaled by 2^256 or 2^261) is 1, 2^29 - 1, 2^29 or p - 1 - at EVERY round, on every lane -
through pmx_permute_batch_dev (the planted states lead the batch, one of them is also the lone lane of the tail wave),
pmx_sponge_squeeze_batch_dev (Absorbing{0}: permute, then squeeze 1 and rate elements; states, outputs and mode words compared) and
pmx_sponge_squeeze_bytes_batch_dev (the canonical cut of output lanes that are exactly 0, p - 1, ...).  pmx_ctx_engine_info is asked
before every call and must name the intended engine.

pmx_sponge_grind meets sponges whose digest for one nonce v is 2^b * odd, b up to B - 2, and exactly 0: it must return v at bits = b
(or the smaller nonce the C port accepts) and not at b + 1 - a kernel that looked at the low 32 or 64 bits alone fails here."""
import ctypes
import functools
import time

import numpy as np
import pytest

import sponge_amd as S
from sponge_amd import _lib
from sponge_amd._lib import MODE_ABSORBING, MODE_SQUEEZING
from oracle import cref

import plants as P

pytestmark = pytest.mark.gpu

QUAD_MAX = 32768           # pmx_device.hip: kQuadMaxUnits
WINDOW_T3_N = QUAD_MAX + 257

# id: (config of tests/plants.py, units of every launch or None = the plants rounded up to 64 k + 1, engine prefix, p = 1 mod 2^29)
INSTANTIATIONS = {
    "quad-bls-a5": ("bls_t3_a5_8_31", None, b"QuadEngine<5>", True),
    "window-t3-p1-a5": ("bls_t3_a5_8_31", WINDOW_T3_N, b"HybridEngine<3,5,", True),
    "window-t3-p1-generic": ("bls_t3_a17_8_31", WINDOW_T3_N, b"HybridEngine<3,0,", True),
    "window-t3-p0-a5": ("bn254_t3_a5_8_57", WINDOW_T3_N, b"HybridEngine<3,5,", False),
    "window-t4-p1-a5": ("bls_t4_a5_8_56", None, b"HybridEngine<4,5,", True),
    "window-t9-p1-a5": ("bls_t9_a5_8_57", None, b"HybridEngine<9,5,", True),
    "window-t9-p0-a5": ("bn254_t9_a5_8_57", None, b"HybridEngine<9,5,", False),
    "runtime-width-t16": ("bls_t16_a5_4_6", None, b"LdsEngine<5>", True),
    "window-t3-top-byte-127": ("p127_t3_a5_8_31", WINDOW_T3_N, b"HybridEngine<3,5,", False),
}


@functools.lru_cache(maxsize=None)
def product_config(name):
    """constants from the PRODUCT's own LFSR"""
    p, bits, rate, alpha, rf, rp = P.parameters(name)
    known = {f.modulus: f for f in (S.BLS12_381_FR, S.BN254_FR)}
    f = known.get(p) or S.Field("prime255_top127", p)
    return S.poseidon_config_from_lfsr(f, rate, alpha, rf, rp)


def units(ident):
    name, n, _, _ = INSTANTIATIONS[ident]
    k = len(P.plants(name).plants)
    if n is None:
        n = (k + 64) // 64 * 64 + 1              # the plants, at least one more unit, and a tail wave of one lane
    assert n > k and n % 64 == 1 and (n <= QUAD_MAX or not ident.startswith("quad"))
    return n


def require_engine(ident, op, n, length=0):
    name, _, prefix, p1 = INSTANTIATIONS[ident]
    cfg = product_config(name)
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(cfg.context(0)._h, op, n, length, ctypes.byref(info)))
    assert info.engine.startswith(prefix), (ident, info.engine)
    assert (cfg.field.modulus % 2**29 == 1) == p1, (ident, "the config's modulus takes the other Montgomery step")


class Device:
    """arrays in buffers of the ABI's own allocator"""

    def __init__(self):
        self.held = []

    def put(self, a):
        lib = _lib.lib()
        a = np.ascontiguousarray(a)
        d = ctypes.c_void_p()
        _lib.check(lib.pmx_device_alloc(0, ctypes.byref(d), max(a.nbytes, 1)))
        self.held.append(d)
        _lib.check(lib.pmx_device_upload(0, d, ctypes.c_void_p(a.ctypes.data), a.nbytes, None))
        return d

    def get(self, d, like):
        lib = _lib.lib()
        back = np.zeros_like(like)
        _lib.check(lib.pmx_device_download(0, ctypes.c_void_p(back.ctypes.data), d, back.nbytes, None))
        _lib.check(lib.pmx_stream_synchronize(0, None))
        return back

    def free(self):
        for d in self.held:
            _lib.check(_lib.lib().pmx_device_free(0, d))
        self.held = []


@functools.lru_cache(maxsize=None)
def batch(ident):
    """(states [n][t][4], the C port's permutation of them): the plants, seeded random states, and the last plant once more as the
    last unit"""
    name = INSTANTIATIONS[ident][0]
    pl = P.plants(name)
    states, want = P.padded(pl, units(ident), seed=0xBA7C4, last=len(pl.plants) - 1)
    states.setflags(write=False)
    want.setflags(write=False)
    return states, want


def differing(got, want):
    return [int(i) for i in np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0]]


def describe(ident, rows):
    pl = P.plants(INSTANTIATIONS[ident][0])
    return [(i, pl.plants[i] if i < len(pl.plants) else "padding") for i in rows[:8]]


@pytest.mark.parametrize("ident", list(INSTANTIATIONS))
def test_permute_batch_dev(ident):
    name = INSTANTIATIONS[ident][0]
    pl = P.plants(name)
    print("%-24s %5d plants generated in %.2f s" % (name, len(pl.plants), pl.seconds))
    states, want = batch(ident)
    n = states.shape[0]
    assert np.array_equal(states[n - 1], pl.inputs[-1]) and (n - 1) % 64 == 0
    require_engine(ident, _lib.OP_PERMUTE, n)
    dev = Device()
    try:
        d = dev.put(states)
        product_config(name).context(0).permute_batch_dev(d.value, n, 0)
        got = dev.get(d, states)
    finally:
        dev.free()
    rows = differing(got, want)
    assert rows == [], (ident, len(rows), "units differ from the C port", describe(ident, rows))


@pytest.mark.parametrize("out_len", ["one", "rate"])
@pytest.mark.parametrize("ident", list(INSTANTIATIONS))
def test_sponge_squeeze_batch_dev(ident, out_len):
    """Absorbing{0}: the squeeze permutes first (mod.rs:324-328), then hands out state[capacity ..]"""
    name = INSTANTIATIONS[ident][0]
    cfg = product_config(name)
    out_len = 1 if out_len == "one" else cfg.rate
    states, _ = batch(ident)
    n = states.shape[0]
    tags = np.full(n, MODE_ABSORBING, dtype=np.uint32)
    indices = np.zeros(n, dtype=np.uint32)
    want_states, want_tags, want_indices, want_out = P.c_port(name).sponge_squeeze_each(states, tags, indices, out_len)
    assert (want_tags == MODE_SQUEEZING).all() and (want_indices == out_len).all()
    require_engine(ident, _lib.OP_SQUEEZE, n, out_len)
    out = np.zeros((n, out_len, 4), dtype=np.uint64)
    dev = Device()
    try:
        d_states, d_tags, d_indices, d_out = dev.put(states), dev.put(tags), dev.put(indices), dev.put(out)
        cfg.context(0).sponge_squeeze_batch_dev(d_states.value, d_tags.value, d_indices.value, d_out.value, out_len, n, 0)
        got_states, got_tags, got_indices, got_out = dev.get(d_states, states), dev.get(d_tags, tags), dev.get(d_indices, indices), dev.get(d_out, out)
    finally:
        dev.free()
    rows = differing(got_states, want_states)
    assert rows == [], (ident, len(rows), "states differ from the C port", describe(ident, rows))
    rows = differing(got_out, want_out)
    assert rows == [], (ident, len(rows), "outputs differ from the C port", describe(ident, rows))
    assert np.array_equal(got_tags, want_tags) and np.array_equal(got_indices, want_indices)


@pytest.mark.parametrize("ident", list(INSTANTIATIONS))
def test_sponge_squeeze_bytes_batch_dev(ident):
    """the output plants (every output lane exactly 0, 1, p - 1, ...), num_bytes = the usable bytes of one element: the first
    (B - 1) / 8 little-endian bytes of the canonical integer of state[capacity] (mod.rs:256-270).  The elements are the C port's; the cut
    is Python integers."""
    name, fixed_n, _, _ = INSTANTIATIONS[ident]
    cfg, pl = product_config(name), P.plants(name)
    p, t = pl.cfg.p, pl.cfg.t
    usable = (P.parameters(name)[1] - 1) // 8
    rows = P.output_plants(pl)
    assert len(rows) == 13 * (1 + t)
    k = len(rows)
    n = fixed_n or (k + 64) // 64 * 64 + 1
    filler, _ = batch(ident)
    states = np.concatenate([pl.inputs[rows], filler[-(n - k):]])
    assert states.shape[0] == n
    tags = np.full(n, MODE_ABSORBING, dtype=np.uint32)
    indices = np.zeros(n, dtype=np.uint32)
    want_states, want_tags, want_indices, elems = P.c_port(name).sponge_squeeze_each(states, tags, indices, 1)
    canon = cref.limbs_to_elems(elems.reshape(n, 4), p)
    planted = {v for _, v in P.edges(p)}
    assert all(canon[i] in planted for i in range(k) if pl.plants[rows[i]].lane in (None, pl.cfg.capacity))
    assert {0, p - 1} <= set(canon[:k])
    want = np.frombuffer(b"".join(v.to_bytes(32, "little")[:usable] for v in canon), dtype=np.uint8).reshape(n, usable)
    require_engine(ident, _lib.OP_SQUEEZE, n, 1)
    out = np.full((n, usable), 0xA5, dtype=np.uint8)
    dev = Device()
    try:
        d_states, d_tags, d_indices, d_out = dev.put(states), dev.put(tags), dev.put(indices), dev.put(out)
        cfg.context(0).sponge_squeeze_bytes_batch_dev(d_states.value, d_tags.value, d_indices.value, d_out.value, usable, n, 0)
        got_states, got_tags, got_indices, got = dev.get(d_states, states), dev.get(d_tags, tags), dev.get(d_indices, indices), dev.get(d_out, out)
    finally:
        dev.free()
    bad = differing(got, want)
    assert bad == [], (ident, len(bad), "byte rows differ", [(i, pl.plants[rows[i]] if i < k else "padding") for i in bad[:8]])
    assert differing(got_states, want_states) == []
    assert np.array_equal(got_tags, want_tags) and np.array_equal(got_indices, want_indices)


# ---- grind on planted digests ---------------------------------------------------------------------------------------------------------
# id: (config, candidates of every search, engine prefix)
GRIND_ENGINES = {
    "quad": ("bls_t3_a5_8_31", 300, b"QuadEngine<5>"),
    "window-t3": ("bls_t3_a5_8_31", QUAD_MAX + 300, b"HybridEngine<3,5,"),
    "window-t9-bn254": ("bn254_t9_a5_8_57", 300, b"HybridEngine<9,5,"),
    "runtime-width-t16": ("bls_t16_a5_4_6", 300, b"LdsEngine<5>"),
}


@pytest.mark.parametrize("b", P.GRIND_BITS, ids=["b%s" % b for b in P.GRIND_BITS])
@pytest.mark.parametrize("mode", ["absorbing1", "squeezing0"])
@pytest.mark.parametrize("engine", list(GRIND_ENGINES))
def test_grind_accepts_exactly_the_planted_zero_bits(engine, mode, b):
    """the digest of nonce v is 2^b * odd: accepted at bits = b, rejected at b + 1; a digest of exactly 0 is accepted at B - 1, the most
    one element yields.  The answers are the C port's first accepted nonce of the range (v, unless a smaller one exists)."""
    name, span, prefix = GRIND_ENGINES[engine]
    cfg = product_config(name)
    state, tag, index, v, first, count, _ = P.grind_case(name, b, mode == "squeezing0", span)
    number, ask = P.grind_bits(name, b)
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(cfg.context(0)._h, _lib.OP_GRIND, count, 0, ctypes.byref(info)))
    assert info.engine.startswith(prefix), (engine, info.engine)
    digests = P.grind_digests(name, state, tag, index, first, count)
    want = P.first_hit(digests, first, ask)
    assert want is not None and want <= v and (want == v or digests[want - first] & ((1 << ask) - 1) == 0)
    st = np.array(state)
    assert cfg.context(0).sponge_grind(st, tag, index, ask, first, count) == want, (engine, mode, b, "bits = %d" % ask)
    assert st.tobytes() == state.tobytes(), "the caller's state was modified"
    if number is not None:
        harder = P.first_hit(digests, first, ask + 1)
        assert harder != v
        assert cfg.context(0).sponge_grind(st, tag, index, ask + 1, first, count) == harder, (engine, mode, b, "bits = %d" % (ask + 1))
