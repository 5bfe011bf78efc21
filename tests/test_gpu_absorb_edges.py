"""Absorbed sums at 0, p, p +- 1 and 2p - 2 on every engine.

Every absorbed element reaches the state through one field addition, `state[capacity + i] += element` (reference
src/poseidon/mod.rs:128,143).  The per-lane kernels (pmx_kernels.hpp: absorb_elements, hash_kernel) add lazily and only
propagate carries - the sum is reduced by the next permutation or, when the call ends without one, by the engine's
to_abi (fe_to_abi_scaled on QuadEngine / HybridEngine, fe_to_abi on LdsEngine); the pass kernels (sponge_walk,
AbsorbAdjust) add the ABI residues with one exact conditional subtraction (abi_add_mod).  A random element meets none of
these edges; tests/absorb_edges.py picks every element from the state it meets, so that raw sums of p, p - 1, p + 1 and
2p - 2 reach every add site, in calls that end with and without a permutation after the last addition.

Every call is preceded by pmx_ctx_engine_info and the engine family it must run on; results are compared limb for limb
(states, outputs, mode words) with the generator's lockstep sponges for the whole batch and, sponge by sponge, with the
C port (every sponge, or a sample of the largest batches)."""
import ctypes

import numpy as np
import pytest

from sponge_amd import _lib
from oracle import poseidon_oracle as O

import absorb_edges as E
from gpu_helpers import c_oracle, product_config
from test_gpu_sponge_passes import P25519, PALLAS, _config, _engine_info, _modes

pytestmark = pytest.mark.gpu

QUAD, PASSES, HYBRID, LDS = "quad", "passes", "hybrid", "lds"


def _family_ok(info, family):
    e = info.engine
    return {QUAD: e.startswith(b"QuadEngine<"),
            PASSES: e.startswith(b"HybridEngine<") and b"passes" in e,
            HYBRID: e.startswith(b"HybridEngine<") and b"passes" not in e,
            LDS: e.startswith(b"LdsEngine<")}[family]


def _expect(cfg, op, n, length, family):
    info = _engine_info(cfg, op, n, length)
    assert _family_ok(info, family), (family, op, n, length, info.engine)


def _named(name):
    return product_config(name), c_oracle(name)


def _custom(modulus, rate, alpha, rf, rp, bits=255):
    """a config of any modulus (and the bls / bn254 fields by value): product side and C port"""
    name = {O.BLS12_381_FR: "bls12_381_fr", O.BN254_FR: "bn254_fr"}.get(modulus)
    _, cfg, cr = _config(name or "custom", None if name else modulus, bits, rate, alpha, rf, rp)
    return cfg, cr


# ---- device-resident calls through the ABI's own memory helpers ---------------------------------------------------------------------
def _to_device(arr):
    lib = _lib.lib()
    p = ctypes.c_void_p()
    _lib.check(lib.pmx_device_alloc(0, ctypes.byref(p), max(arr.nbytes, 32)))
    if arr.nbytes:
        _lib.check(lib.pmx_device_upload(0, p, ctypes.c_void_p(arr.ctypes.data), arr.nbytes, None))
    return p


def _sponge_call_dev(cfg, squeeze, state, tag, idx, io, length):
    """one _dev absorb (io = the elements) or squeeze (io = the output buffer) on device copies; results copied back in place"""
    lib = _lib.lib()
    n = tag.shape[0]
    bufs = [_to_device(np.ascontiguousarray(x)) for x in (state, tag, idx, io)]
    try:
        _lib.check(lib.pmx_stream_synchronize(0, None))
        call = cfg.context().sponge_squeeze_batch_dev if squeeze else cfg.context().sponge_absorb_batch_dev
        call(bufs[0].value, bufs[1].value, bufs[2].value, bufs[3].value, length, n, 0)
        for host, dev in zip((state, tag, idx, io), bufs):
            if host.nbytes:
                _lib.check(lib.pmx_device_download(0, ctypes.c_void_p(host.ctypes.data), dev, host.nbytes, None))
        _lib.check(lib.pmx_stream_synchronize(0, None))
    finally:
        for b in bufs:
            lib.pmx_device_free(0, b)


def _run_script(cfg, cr, n, script, family, dev=False, layout="random", sample=None, seed=1):
    """n sponges from edge start states in mixed modes through `script`, every call against the generator's lockstep sponges
    (whole batch) and the C port (sponge by sponge: all, or `sample`)"""
    ocfg, p, r, t = cr.cfg, cr.cfg.p, cfg.rate, cfg.rate + cfg.capacity
    st0 = E.edge_states(p, n, t, seed)
    tag0, idx0 = E.mixed_modes(n, r, seed) if layout == "random" else _modes(n, r, layout, np.random.default_rng(seed))
    g = E.EdgeSponges(ocfg, st0, tag0, idx0, seed=seed, c_port=cr)
    state, tag, idx = st0.copy(), tag0.copy(), idx0.copy()
    check = range(n) if sample is None else sample
    ref = {int(j): (st0[j].copy(), int(tag0[j]), int(idx0[j])) for j in check}
    ctx = cfg.context()
    for step, (op, length) in enumerate(script):
        _expect(cfg, _lib.OP_ABSORB if op == "absorb" else _lib.OP_SQUEEZE, n, length, family)
        if op == "absorb":
            elems = g.absorb(length)
            if dev:
                _sponge_call_dev(cfg, False, state, tag, idx, elems, length)
            else:
                ctx.sponge_absorb_batch(state, tag, idx, elems, length)
            for j, (s, m, i) in ref.items():
                ref[j] = cr.sponge_absorb(s, m, i, elems[j])
        else:
            want = g.squeeze(length)
            if dev:
                out = np.zeros((n, length, 4), dtype=np.uint64)
                _sponge_call_dev(cfg, True, state, tag, idx, out, length)
            else:
                out = ctx.sponge_squeeze_batch(state, tag, idx, length)
            bad = np.nonzero((out != want).any(axis=(1, 2)))[0]
            assert bad.size == 0, (op, length, step, bad[:8])
            for j, (s, m, i) in ref.items():
                s2, m2, i2, o = cr.sponge_squeeze(s, m, i, length)
                assert np.array_equal(out[j], o), (op, length, step, j)
                ref[j] = (s2, m2, i2)
        bad = np.nonzero((state != g.state).any(axis=(1, 2)))[0]
        assert bad.size == 0, (op, length, step, bad[:8], [g.adds[-1]])
        assert np.array_equal(tag, g.tag) and np.array_equal(idx, g.idx), (op, length, step)
        for j, (s, m, i) in ref.items():
            assert np.array_equal(state[j], s) and (int(tag[j]), int(idx[j])) == (m, i), (op, length, step, j)
    return g


def _script(r):
    """absorbs of 1, r - 1, r (from Absorbing{0} these end without a permutation after the last add), r + 1, 2r + 2 and > 10 rates
    (lane resets after every permutation), squeezes in between that read the states back"""
    ops = [("absorb", 1), ("absorb", r), ("squeeze", 1), ("absorb", r + 1), ("absorb", 2 * r + 2), ("squeeze", r),
           ("absorb", 10 * r + 1), ("squeeze", 2 * r + 1), ("absorb", 1), ("squeeze", 1)]
    if r > 1:
        ops.insert(1, ("absorb", r - 1))
    return ops


def _check_hits(g):
    assert all(g.hits[k] > 0 for k in E.ALL_HITS), g.hits


# ---- QuadEngine: t = 3, rate 2, capacity 1, at most 32768 units ---------------------------------------------------------------------
QUAD_CONFIGS = {
    "bls-a5": lambda: _named("bls_t3_a5_8_31"),
    "bls-a17": lambda: _named("bls_t3_a17_8_31"),        # the reference's default rate-2 config
    "bls-a257": lambda: _named("bls_t3_a257_8_13"),      # a generic exponent
    "bn254-a5": lambda: _named("bn254_t3_a5_8_57"),
    "pallas-a5": lambda: _custom(PALLAS, 2, 5, 8, 56),
    "p25519-a5": lambda: _custom(P25519, 2, 5, 8, 56),
}


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("n", [1, 63, 65, 200])
@pytest.mark.parametrize("name", list(QUAD_CONFIGS))
def test_quad_engine_absorb_edges(name, n, dev):
    """n = 1 is the packed small call PoseidonSponge makes; 63, 65, 200 leave a ragged last workgroup of 64 units.  Mixed modes in
    one wave: some quads permute while their neighbours do not."""
    cfg, cr = QUAD_CONFIGS[name]()
    g = _run_script(cfg, cr, n, _script(2), QUAD, dev=dev, seed=n + 17 * dev)
    if n >= 63:
        _check_hits(g)


@pytest.mark.parametrize("name", list(QUAD_CONFIGS))
def test_quad_engine_hash_edges(name):
    """the hash driver (absorb then squeeze in one kernel) with in_len > rate: first blocks of 0 and p - 1, later ones from the state"""
    cfg, cr = QUAD_CONFIGS[name]()
    for n, in_len, out_len in ((200, 7, 3), (65, 3, 1)):
        msgs, want, g = E.hash_rows(cr.cfg, n, in_len, out_len, seed=in_len, c_port=cr)
        _expect(cfg, _lib.OP_HASH, n, 0, QUAD)
        got = cfg.context().hash_batch(msgs, in_len, out_len)
        assert np.array_equal(got, want) and np.array_equal(got, cr.hash_batch(msgs, in_len, out_len, threads=0)), (n, in_len)


# ---- HybridEngine: absorb / squeeze as passes ----------------------------------------------------------------------------------------
def _big_sample(n, seed):
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([np.arange(256), np.arange(n - 256, n), rng.integers(0, n, 300)]))


@pytest.mark.parametrize("name,n", [("bls-a5", 32769), ("bls-a5", 40000), ("bls-a17", 40000), ("pallas-a5", 32769), ("p25519-a5", 32769)])
def test_t3_passes_above_the_quad_range_absorb_edges(name, n):
    """t = 3 above 32768 units: the pass kernels' three add sites (AbsorbAdjust in sponge_first_kernel and permute_listed_kernel, the
    trailing in-memory add of sponge_walk); the whole batch against the lockstep sponges, a sample against the C port"""
    cfg, cr = QUAD_CONFIGS[name]()
    script = [("absorb", 1), ("absorb", 1), ("absorb", 2), ("squeeze", 1), ("absorb", 3), ("absorb", 6), ("squeeze", 2)]
    g = _run_script(cfg, cr, n, script, PASSES, sample=_big_sample(n, n), seed=n)
    _check_hits(g)


WIDE_CONFIGS = {
    "bls-t5-a5": lambda: _custom(O.BLS12_381_FR, 4, 5, 8, 56),
    "bn254-t9-a5": lambda: _named("bn254_t9_a5_8_57"),
    "bls-t9-a17": lambda: _custom(O.BLS12_381_FR, 8, 17, 8, 57),
    "pallas-t9-a5": lambda: _custom(PALLAS, 8, 5, 8, 57),
    "p25519-t9-a5": lambda: _custom(P25519, 8, 5, 8, 57),
    "bls-t3-rf300-rp8": lambda: _custom(O.BLS12_381_FR, 2, 5, 300, 8),  # beyond the quad kernels' LDS: the window engine's passes at any size
}


@pytest.mark.parametrize("layout", ["random", "blocks"])
@pytest.mark.parametrize("name", list(WIDE_CONFIGS))
def test_wide_passes_absorb_edges(name, layout):
    """t = 5, 9: more than two workgroups (the last ragged), calls of one pass, several listed passes and none"""
    cfg, cr = WIDE_CONFIGS[name]()
    g = _run_script(cfg, cr, 2 * 256 + 77, _script(cfg.rate), PASSES, layout=layout, seed=len(name) + (layout == "blocks"))
    _check_hits(g)


@pytest.mark.parametrize("name", ["bn254-t9-a5", "p25519-t9-a5"])
def test_wide_hash_kernel_absorb_edges(name):
    """hash_kernel on HybridEngine: its lazy add, at t = 9, in_len > 2 rates"""
    cfg, cr = WIDE_CONFIGS[name]()
    n, in_len, out_len = 300, 19, 9
    msgs, want, g = E.hash_rows(cr.cfg, n, in_len, out_len, seed=9, c_port=cr)
    _expect(cfg, _lib.OP_HASH, n, 0, HYBRID)
    got = cfg.context().hash_batch(msgs, in_len, out_len)
    assert np.array_equal(got, want) and np.array_equal(got, cr.hash_batch(msgs, in_len, out_len, threads=0))


# ---- LdsEngine: t = 2, t >= 10, and configs whose round constants exceed LDS ------------------------------------------------------
LDS_CONFIGS = {
    "bls-t2-a5": lambda: _custom(O.BLS12_381_FR, 1, 5, 8, 31),
    "bls-t2-a17": lambda: _custom(O.BLS12_381_FR, 1, 17, 8, 31),
    "bn254-t12-a5": lambda: _custom(O.BN254_FR, 11, 5, 8, 57, bits=254),
    "bls-t12-a17": lambda: _custom(O.BLS12_381_FR, 11, 17, 8, 57),
    "bls-t3-rf300": lambda: _custom(O.BLS12_381_FR, 2, 5, 300, 0),      # round constants beyond the quad kernels' LDS, no partial section
}


@pytest.mark.parametrize("name", list(LDS_CONFIGS))
def test_lds_engine_absorb_and_hash_edges(name):
    cfg, cr = LDS_CONFIGS[name]()
    n = 200
    g = _run_script(cfg, cr, n, _script(cfg.rate), LDS, dev=name.endswith("a17"), seed=3)
    _check_hits(g)
    in_len = 2 * cfg.rate + 3
    msgs, want, _ = E.hash_rows(cr.cfg, n, in_len, 3, seed=4, c_port=cr)
    _expect(cfg, _lib.OP_HASH, n, 0, LDS)
    got = cfg.context().hash_batch(msgs, in_len, 3)
    assert np.array_equal(got, want) and np.array_equal(got, cr.hash_batch(msgs, in_len, 3, threads=0))


# ---- compression: no addition, the same conversions -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bls-a5", "bn254-a5", "pallas-a5", "p25519-a5"])
def test_compression_of_edge_leaves_on_quad_and_wide_levels(name):
    """leaves 0, 1, p - 2, p - 1 (every pair of them) through merkle_2to1 - 2^17 leaves: the first level on the pass engine's width
    (65536 compressions), the next ones on the quad kernels - and through the in_len = 2, out_len = 1 hash path on both sides"""
    cfg, cr = QUAD_CONFIGS[name]()
    p = cr.cfg.p
    edge = [0, 1, p - 2, p - 1]
    m = 1 << 17
    vals = [edge[(k >> 1) & 3] if k % 2 == 0 else edge[(k >> 3) & 3] for k in range(m)]   # every ordered pair of edges, over and over
    leaves = E.to_limbs(vals)
    nodes, root = cfg.context().merkle_2to1(leaves)
    want = cr.merkle(leaves, threads=0)
    assert np.array_equal(nodes, want) and np.array_equal(root, want[-1])
    for rows in (64, 40000):
        family = QUAD if rows <= 32768 else HYBRID
        _expect(cfg, _lib.OP_COMPRESS, rows, 0, family)
        msgs = np.ascontiguousarray(leaves[:2 * rows].reshape(rows, 2, 4))
        got = cfg.context().hash_batch(msgs, 2, 1)
        assert np.array_equal(got, cr.hash_batch(msgs, 2, 1, threads=0)), rows


# ---- device-resident mode words out of range --------------------------------------------------------------------------------------
MODE_CASES = [("quad", "bls-a5", 200), ("passes-t3", "bls-a5", 32769), ("passes-t9", "bn254-t9-a5", 300), ("lds", "bls-t2-a5", 200),
              ("lds-t12", "bn254-t12-a5", 200)]


@pytest.mark.parametrize("squeeze", [False, True], ids=["absorb", "squeeze"])
@pytest.mark.parametrize("case", MODE_CASES, ids=lambda c: c[0])
def test_device_resident_mode_words_out_of_range_on_every_engine(case, squeeze):
    """The _dev entry points take mode words the host never validated: an index above the rate is the rate; absorb takes any tag but
    Absorbing as Squeezing, squeeze any tag but Squeezing as Absorbing.  Expected: the C port on the normalised mode words, and the
    tag written back always 0 or 1."""
    label, name, n = case
    cfg, cr = {**QUAD_CONFIGS, **WIDE_CONFIGS, **LDS_CONFIGS}[name]()
    r, t, p = cfg.rate, cfg.rate + cfg.capacity, cr.cfg.p
    family = {"quad": QUAD, "passes-t3": PASSES, "passes-t9": PASSES, "lds": LDS, "lds-t12": LDS}[label]
    length = r + 2
    _expect(cfg, _lib.OP_SQUEEZE if squeeze else _lib.OP_ABSORB, n, length, family)
    rng = np.random.default_rng(n + squeeze)
    st = E.edge_states(p, n, t, seed=n)
    tag = rng.choice(np.array([0, 1, 2, 0xFFFFFFFF], dtype=np.uint32), n).astype(np.uint32)
    idx = rng.choice(np.array([0, 1, r, r + 1, r + 5, 0xFFFFFFFF], dtype=np.uint32), n).astype(np.uint32)
    tag[:4], idx[:4] = [2, 0xFFFFFFFF, 0, 1], [r + 1, 0, r + 5, 0xFFFFFFFF]
    io = np.zeros((n, length, 4), dtype=np.uint64)
    if not squeeze:
        io = E.edge_states(p, n, length, seed=n + 1)
    elems = io.copy()
    got_st, got_tag, got_idx = st.copy(), tag.copy(), idx.copy()
    _sponge_call_dev(cfg, squeeze, got_st, got_tag, got_idx, io, length)
    keep = E.SQUEEZING if squeeze else E.ABSORBING
    sample = range(n) if n <= 300 else _big_sample(n, 5)
    for j in sample:
        m = keep if tag[j] == keep else 1 - keep
        i = min(int(idx[j]), r)
        if squeeze:
            s, m2, i2, o = cr.sponge_squeeze(st[j], m, i, length)
            assert np.array_equal(io[j], o), j
        else:
            s, m2, i2 = cr.sponge_absorb(st[j], m, i, elems[j])
        assert np.array_equal(got_st[j], s) and (int(got_tag[j]), int(got_idx[j])) == (m2, i2), (j, int(tag[j]), int(idx[j]))
    assert set(int(x) for x in got_tag) == {keep}
