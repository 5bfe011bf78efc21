"""squeeze_bytes / squeeze_bits of device-resident sponge batches (pmx_sponge_squeeze_{bytes,bits}_batch[_dev]) against the reference's
semantics, src/poseidon/mod.rs:256-286.

Where the expected values come from: the native elements of every sponge from the C restatement (oracle/cref.py: CRef.sponge_squeeze per
sponge, permute_batch for the full-size batches), the final states and mode words from the same calls; the cut into bytes and bits is
Python integer arithmetic written here from mod.rs:256-286 (`canonical = residue * 2^-256 mod p`, little-endian, the first u bytes /
bits of every element, the concatenation truncated).  The reference holds no known answer for squeeze_bytes: the result is a pure
function of the native elements, which are pinned, and of ark-ff's little-endian into_bigint.

Every _dev call runs in a guard-band arena (tests/arena.py): d_out at an odd address, states at 16 mod 32, mode words at 4 mod 8, 256 KiB
of poisoned guard around each; no byte outside d_out, the states and the mode words may change, and all three are compared in full."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import sponge_amd as S
from sponge_amd import _lib, synth
from oracle import cref
from oracle import poseidon_oracle as O

import arena

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

P25519 = (1 << 255) - 19
P248 = (1 << 248) - 237      # a 248-bit prime: u = 30 bytes / 247 bits
SCRATCH_CAP = 64 << 20       # PMX_SQUEEZE_SCRATCH_BYTES (include/poseidon_mi355x.h)
QUAD_MAX = 32768

# label: (field name, modulus or None, prime bits, rate, alpha, RF, RP, batch size, engine name prefix)
CONFIGS = {
    "quad-t3": ("bls12_381_fr", None, 255, 2, 5, 8, 31, 700, b"QuadEngine"),
    "window-t3": ("bls12_381_fr", None, 255, 2, 5, 8, 31, QUAD_MAX + 300, b"HybridEngine<3,5"),
    "window-t4": ("bls12_381_fr", None, 255, 3, 5, 8, 56, 600, b"HybridEngine<4,5"),
    "window-t5": ("bls12_381_fr", None, 255, 4, 5, 8, 56, 600, b"HybridEngine<5,5"),
    "window-t6": ("bls12_381_fr", None, 255, 5, 5, 8, 57, 600, b"HybridEngine<6,5"),
    "window-t7": ("bls12_381_fr", None, 255, 6, 5, 8, 57, 600, b"HybridEngine<7,5"),
    "window-t8": ("bls12_381_fr", None, 255, 7, 5, 8, 57, 600, b"HybridEngine<8,5"),
    "window-t9-bn254": ("bn254_fr", None, 254, 8, 5, 8, 57, 600, b"HybridEngine<9,5"),
    "window-t9-alpha17": ("bls12_381_fr", None, 255, 8, 17, 8, 57, 600, b"HybridEngine<9,0"),
    "window-t9-p25519": ("p25519", P25519, 255, 8, 5, 8, 57, 600, b"HybridEngine<9,5"),
    "quad-t3-p25519": ("p25519", P25519, 255, 2, 5, 8, 31, 600, b"QuadEngine"),
    "quad-t3-p248": ("p248", P248, 248, 2, 5, 8, 31, 600, b"QuadEngine"),
    "window-t9-p248": ("p248", P248, 248, 8, 5, 8, 57, 600, b"HybridEngine<9,5"),
    "rt-t2": ("bls12_381_fr", None, 255, 1, 5, 8, 31, 600, b"LdsEngine"),
    "rt-t16": ("bls12_381_fr", None, 255, 15, 5, 4, 6, 600, b"LdsEngine"),
}
ENGINES_SEEN = set()


@functools.lru_cache(maxsize=None)
def _config(label):
    field_name, modulus, bits, rate, alpha, rf, rp, _, _ = CONFIGS[label]
    f = S.FIELDS[field_name] if modulus is None else S.Field(field_name, modulus)
    return f, S.poseidon_config_from_lfsr(f, rate, alpha, rf, rp), cref.CRef(O.make_config(f.modulus, bits, rate, alpha, rf, rp))


def _units(p):
    """(usable bytes, usable bits) of one element: mod.rs:257, 274"""
    return (p.bit_length() - 1) // 8, p.bit_length() - 1


def _elems_for(length, unit):
    return (length + unit - 1) // unit          # mod.rs:258, 275


def _engine(cfg, n, elems):
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(cfg.context()._h, _lib.OP_SQUEEZE, n, elems, ctypes.byref(info)))
    return info


# ---- the reference -------------------------------------------------------------------------------------------------------------
def _ref_squeeze(cr, states, tag, index, elems):
    """CRef.sponge_squeeze of every sponge: (elements [n][elems][4], states, tags, indices)"""
    n = states.shape[0]

    def one(i):
        return cr.sponge_squeeze(states[i], int(tag[i]), int(index[i]), elems)
    with ThreadPoolExecutor(16) as pool:
        res = list(pool.map(one, range(n), chunksize=64))
    out = np.stack([r[3] for r in res]).reshape(n, elems, 4) if elems else np.zeros((n, 0, 4), dtype=np.uint64)
    return (out, np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.uint32),
            np.array([r[2] for r in res], dtype=np.uint32))


def _canonical_bytes(p, elements):
    """[...][4] u64 Montgomery residues -> [...][32] u8: the little-endian bytes of  residue * 2^-256 mod p  (into_bigint)"""
    rinv = pow(1 << 256, -1, p)
    flat = np.ascontiguousarray(elements, dtype=np.uint64).reshape(-1, 4)
    raw = flat.tobytes()
    out = bytearray(len(raw))
    for i in range(flat.shape[0]):
        a = int.from_bytes(raw[32 * i:32 * i + 32], "little")
        out[32 * i:32 * i + 32] = (a * rinv % p).to_bytes(32, "little")
    return np.frombuffer(bytes(out), dtype=np.uint8).reshape(elements.shape[:-1] + (32,))


def _cut(p, elements, length, bits):
    """mod.rs:256-286 on the native elements [n][E][4]: [n][length] u8 (bits: one byte per bit)"""
    n = elements.shape[0]
    ub, ubits = _units(p)
    canon = _canonical_bytes(p, elements)                                        # [n][E][32]
    if bits:
        per = np.unpackbits(canon, axis=-1, bitorder="little")[:, :, :ubits]     # to_bits_le()[..usable_bits]
    else:
        per = canon[:, :, :ub]                                                   # to_bytes_le()[..usable_bytes]
    return np.ascontiguousarray(per.reshape(n, -1)[:, :length])                  # truncate(num)


# ---- sponges and device arenas -------------------------------------------------------------------------------------------------------
def _sponges(f, cfg, n, seed):
    """n sponges with seeded states, in every mode: Absorbing{0 .. rate} and Squeezing{0 .. rate}, all of them present"""
    rate = cfg.rate
    rng = np.random.default_rng(seed)
    states = synth.random_elements(f, n * cfg.t, seed=seed).reshape(n, cfg.t, 4)
    tag = rng.integers(0, 2, n).astype(np.uint32)
    index = rng.integers(0, rate + 1, n).astype(np.uint32)
    modes = [(m, i) for m in (0, 1) for i in range(rate + 1)]
    for k, (m, i) in enumerate(modes):
        if k < n:
            tag[k], index[k] = m, i
    if n >= len(modes):
        assert {(int(a), int(b)) for a, b in zip(tag, index)} == set(modes)
    return states, tag, index


def _buffers(t, n, length):
    return [("d_states", n * t * 32, 16, "inout"), ("d_mode_tag", n * 4, 4, "inout"), ("d_mode_index", n * 4, 4, "inout"),
            ("d_out", n * length, 1, "out")]


class DeviceArena:
    """the buffers of one call in one device allocation (tests/arena.py), poisoned; a clone to compare with"""

    def __init__(self, buffers, seed):
        self.plan = arena.plan(buffers)
        self.image = self.plan.poisoned(seed)

    def put(self, name, data):
        self.plan.put(self.image, name, data)

    def upload(self):
        self.dev = torch.from_numpy(self.image).to("cuda:0")
        arena.assert_base_aligned(self.dev.data_ptr())
        self.before = self.dev.clone()
        torch.cuda.synchronize()
        for r in self.plan.regions:
            assert self.ptr(r.name) % (2 * r.align) == r.align, (r.name, hex(self.ptr(r.name)))   # d_out: odd
        return self

    def ptr(self, name):
        return self.plan.address(self.dev.data_ptr(), name)

    def finish(self):
        torch.cuda.synchronize()
        self.plan.check(self.before, self.dev)

    def unchanged(self):
        torch.cuda.synchronize()
        assert torch.equal(self.before, self.dev), "the call changed the arena"

    def get(self, name, dtype):
        return self.plan.get(self.dev, name, dtype)


def _dev_arena(cfg, states, tag, index, length, seed):
    n = tag.shape[0]
    a = DeviceArena(_buffers(cfg.t, n, length), seed)
    a.put("d_states", states)
    a.put("d_mode_tag", tag)
    a.put("d_mode_index", index)
    return a.upload()


def _call_dev(cfg, a, length, n, bits, stream=None):
    fn = _lib.lib().pmx_sponge_squeeze_bits_batch_dev if bits else _lib.lib().pmx_sponge_squeeze_bytes_batch_dev
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    return fn(cfg.context()._h, a.ptr("d_states"), a.ptr("d_mode_tag"), a.ptr("d_mode_index"), a.ptr("d_out"), length, n, s)


def _check_dev(cfg, a, want_out, want_states, want_tag, want_index, bits, what):
    a.finish()                                                       # no guard byte changed
    n, length = want_out.shape
    got = a.get("d_out", np.uint8).reshape(n, length)
    if bits:
        assert int(got.max(initial=0)) <= 1, (what, "a bit byte is neither 0 nor 1")
    bad = np.nonzero((got != want_out).any(axis=1))[0]
    assert bad.size == 0, (what, "rows differ", bad[:8])
    st = a.get("d_states", np.uint64).reshape(want_states.shape)
    bad = np.nonzero((st != want_states).any(axis=(1, 2)))[0]
    assert bad.size == 0, (what, "states differ", bad[:8])
    assert np.array_equal(a.get("d_mode_tag", np.uint32), want_tag), (what, "tags")
    assert np.array_equal(a.get("d_mode_index", np.uint32), want_index), (what, "indices")


def _lengths(unit, rate, seed):
    """0, 1, u - 1, u, u + 1, rate u, rate u + 1, 2 rate u (the :175 case: E = rate from inside the rate) and two seeded odd lengths"""
    rng = np.random.default_rng(seed)
    odd = [int(v) | 1 for v in rng.integers(2, 3 * rate * unit, 2)]
    return [0, 1, unit - 1, unit, unit + 1, rate * unit, rate * unit + 1, 2 * rate * unit] + odd


# ---- every engine, every modulus, every mode, every length: host and _dev, bytes and bits ------------------------------------------
@pytest.mark.parametrize("label", sorted(CONFIGS))
def test_bytes_and_bits_in_every_mode_and_length(label):
    f, cfg, cr = _config(label)
    p, rate, n = f.modulus, cfg.rate, CONFIGS[label][7]
    states, tag, index = _sponges(f, cfg, n, seed=0xB17E5 + rate)
    ub, ubits = _units(p)
    assert _lib.lib().pmx_abi_version() == 5
    refs = {}
    for bits, unit in ((False, ub), (True, ubits)):
        lengths = _lengths(unit, rate, seed=rate * 7 + bits)
        for length in lengths:
            elems = _elems_for(length, unit)
            info = _engine(cfg, n, elems)
            assert info.engine.startswith(CONFIGS[label][8]), (label, info.engine)
            ENGINES_SEEN.add(info.engine.split(b"<")[0])
            if elems not in refs:
                refs[elems] = _ref_squeeze(cr, states, tag, index, elems)
            el, want_states, want_tag, want_index = refs[elems]
            want = _cut(p, el, length, bits)
            assert want.shape == (n, length)
            what = (label, "bits" if bits else "bytes", length)
            # the host entry, through the batch type
            batch = S.BatchPoseidonSponge.from_state((states, tag, index), cfg)
            got = batch.squeeze_bits(length) if bits else batch.squeeze_bytes(length)
            assert got.shape == (n, length) and got.dtype == (np.bool_ if bits else np.uint8)
            bad = np.nonzero((got.view(np.uint8) != want).any(axis=1))[0]
            assert bad.size == 0, (what, "host rows differ", bad[:8])
            assert np.array_equal(batch.state, want_states), (what, "host states")
            assert np.array_equal(batch.mode_tag, want_tag) and np.array_equal(batch.mode_index, want_index), (what, "host modes")
            # the _dev entry, in the arena
            a = _dev_arena(cfg, states, tag, index, length, seed=length + 17)
            _lib.check(_call_dev(cfg, a, length, n, bits))
            _check_dev(cfg, a, want, want_states, want_tag, want_index, bits, what)


def test_every_engine_was_seen():
    """the three engine names, asked of pmx_ctx_engine_info(PMX_OP_SQUEEZE, n, E) for the calls the test above makes"""
    seen = set()
    for label in CONFIGS:
        f, cfg, cr = _config(label)
        seen.add(_engine(cfg, CONFIGS[label][7], 2).engine.split(b"<")[0])
    assert seen == {b"QuadEngine", b"HybridEngine", b"LdsEngine"}, seen
    assert not ENGINES_SEEN or ENGINES_SEEN == seen, (ENGINES_SEEN, seen)


# ---- full size ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,field_name,bits,rate,rp,n", [("t3", "bls12_381_fr", 255, 2, 31, 1 << 20), ("t9", "bn254_fr", 254, 8, 57, 1 << 18)])
def test_full_size_batch_of_32_bytes(label, field_name, bits, rate, rp, n):
    """2^20 (t = 3) / 2^18 (t = 9) Absorbing sponges, 32 bytes each (E = 2): states and mode words in full against the C port's
    permutation of the same states (an Absorbing sponge permutes once and squeezes from 0, mod.rs:324-328), the bytes of a seeded sample
    of 4096 sponges against the C port's elements, every row for internal consistency: no row of zeros, no two equal rows."""
    f = S.FIELDS[field_name]
    cfg = S.poseidon_config_from_lfsr(f, rate, 5, 8, rp)
    cr = cref.CRef(O.make_config(f.modulus, bits, rate, 5, 8, rp))
    t, p = cfg.t, f.modulus
    assert _elems_for(32, _units(p)[0]) == 2 and n * 2 * 32 <= SCRATCH_CAP
    assert b"HybridEngine" in _engine(cfg, n, 2).engine
    states = synth.random_elements(f, n * t, seed=0xF011 + t).reshape(n, t, 4)
    rng = np.random.default_rng(t)
    tag = np.zeros(n, dtype=np.uint32)
    index = rng.integers(0, rate + 1, n).astype(np.uint32)
    a = _dev_arena(cfg, states, tag, index, 32, seed=5)
    _lib.check(_call_dev(cfg, a, 32, n, False))
    a.finish()
    want_states = cr.permute_batch(states, threads=0)
    assert np.array_equal(a.get("d_states", np.uint64).reshape(n, t, 4), want_states)
    assert np.array_equal(a.get("d_mode_tag", np.uint32), np.ones(n, dtype=np.uint32))
    assert np.array_equal(a.get("d_mode_index", np.uint32), np.full(n, 2, dtype=np.uint32))
    got = a.get("d_out", np.uint8).reshape(n, 32)
    sample = np.sort(rng.choice(n, 4096, replace=False))
    el = np.ascontiguousarray(want_states[sample, cfg.capacity:cfg.capacity + 2])      # the C port's squeezed elements
    one = cr.sponge_squeeze(states[sample[0]], 0, int(index[sample[0]]), 2)
    assert np.array_equal(one[3].reshape(2, 4), el[0])
    assert np.array_equal(got[sample], _cut(p, el, 32, False))
    assert int((got != 0).any(axis=1).sum()) == n, "a row of zeros"
    assert np.unique(np.ascontiguousarray(got).view(np.uint64), axis=0).shape[0] == n, "two equal rows"


# ---- a call above the scratch cap: slices over sponges -------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [False, True], ids=["bytes", "bits"])
def test_call_above_the_scratch_cap_is_sliced(bits):
    """2^16 sponges x 40 elements = 80 MiB of native elements against a cap of 64 MiB: the call runs in two slices over sponges
    (52428 and 13108 of them: the window engine and the quad engine).  Mixed modes; everything checked in full."""
    label = "quad-t3"
    f, cfg, cr = _config(label)
    n, elems, p = 1 << 16, 40, f.modulus
    assert n * elems * 32 > SCRATCH_CAP
    unit = _units(p)[1 if bits else 0]
    length = (elems - 1) * unit + unit // 2 + 1                 # the last element truncated, an odd row length for bytes
    assert _elems_for(length, unit) == elems
    states, tag, index = _sponges(f, cfg, n, seed=0x511CE)
    el, want_states, want_tag, want_index = _ref_squeeze(cr, states, tag, index, elems)
    want = _cut(p, el, length, bits)
    a = _dev_arena(cfg, states, tag, index, length, seed=9)
    _lib.check(_call_dev(cfg, a, length, n, bits))
    _check_dev(cfg, a, want, want_states, want_tag, want_index, bits, ("sliced", bits))


# ---- limits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [False, True], ids=["bytes", "bits"])
def test_dev_refuses_more_than_65536_rates_and_writes_nothing(bits):
    f, cfg, cr = _config("quad-t3")
    unit = _units(f.modulus)[1 if bits else 0]
    n = 3
    states, tag, index = _sponges(f, cfg, n, seed=3)
    most = 65536 * cfg.rate * unit
    a = _dev_arena(cfg, states, tag, index, 64, seed=1)         # (d_out is not read: the call fails on its arguments)
    assert _call_dev(cfg, a, most + 1, n, bits) == _lib.PMX_ERR_ARG
    assert b"65536 rates" in _lib.lib().pmx_last_error()
    a.unchanged()


@pytest.mark.parametrize("label,n,bits", [("quad-t3", 1, False), ("quad-t3", 3, False), ("window-t4", 3, False), ("quad-t3", 3, True)])
def test_host_entry_takes_more_than_65536_rates(label, n, bits):
    """65536 rate u + 1 bytes (bits) per sponge: one element more than a device call moves.  The host entry cuts the call on an element
    boundary (65536 rates, then one element - never a last piece of exactly one rate), the truncation falls into the last piece, and
    every piece comes down into its columns of the rows."""
    f, cfg, cr = _config(label)
    p, rate = f.modulus, cfg.rate
    unit = _units(p)[1 if bits else 0]
    length = 65536 * rate * unit + 1
    elems = _elems_for(length, unit)
    assert elems == 65536 * rate + 1
    states, tag, index = _sponges(f, cfg, n, seed=0x10)
    el, want_states, want_tag, want_index = _ref_squeeze(cr, states, tag, index, elems)
    want = _cut(p, el, length, bits)
    batch = S.BatchPoseidonSponge.from_state((states, tag, index), cfg)
    got = batch.squeeze_bits(length) if bits else batch.squeeze_bytes(length)
    assert np.array_equal(got.view(np.uint8), want)
    assert np.array_equal(batch.state, want_states)
    assert np.array_equal(batch.mode_tag, want_tag) and np.array_equal(batch.mode_index, want_index)


# ---- two streams of one context -------------------------------------------------------------------------------------------------
def test_two_dev_calls_on_two_streams_of_one_context():
    """each call takes its own scratch block from the context's pool: both results are correct"""
    f, cfg, cr = _config("window-t9-bn254")
    p = f.modulus
    ub = _units(p)[0]
    n, length = 5000, 3 * ub + 5
    elems = _elems_for(length, ub)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    jobs = []
    for k, stream in enumerate((s1, s2)):
        states, tag, index = _sponges(f, cfg, n, seed=0x2000 + k)
        a = _dev_arena(cfg, states, tag, index, length, seed=40 + k)
        jobs.append((states, tag, index, a, stream))
    torch.cuda.synchronize()
    for states, tag, index, a, stream in jobs:
        _lib.check(_call_dev(cfg, a, length, n, False, stream=stream.cuda_stream))
    for states, tag, index, a, stream in jobs:
        stream.synchronize()
    for k, (states, tag, index, a, stream) in enumerate(jobs):
        el, want_states, want_tag, want_index = _ref_squeeze(cr, states, tag, index, elems)
        _check_dev(cfg, a, _cut(p, el, length, False), want_states, want_tag, want_index, False, ("stream", k))
