"""The memory footprint of every *_dev entry point of include/poseidon_mi355x.h, on every engine that serves it (tests/arena.py).

All buffers of a call are carved out of ONE device allocation, at the documented alignment and nothing above it (16-byte buffers at
16 mod 32, u64 arrays at 8 mod 16, mode words at 4 mod 8, d_ok at an odd address), 256 KiB of guard around each, everything poisoned
with random bytes first.  After the call (a) every out / inout buffer equals the C port (oracle/cref) in full - an element a kernel
forgets to write still holds poison - and (b) every byte outside the regions the call may write is unchanged: guards, `const` inputs,
the leaves rows of a node array.  A stray write lands inside the arena and is reported; nothing here can leave the allocation.

Engines (asked of pmx_ctx_engine_info before every call and asserted): the quad engine (t = 3 up to 32768 units), the window engines
(t = 3 from 32769 units, t = 4, 6, 9 at alpha = 5, t = 9 on the generic S-box at alpha = 17), the run-time-width engine at t = 2 and at
t = 16, the widest state (the guard's worst case).  test_no_engine_x_entry_point_cell_is_empty checks the case tables against that list.

Cost.  The C port is the expense, so the full cross product is not run: every entry point takes ALL batch sizes (1, 63, 65, 257, 1000;
t = 3 also 32768 and 32769, the two sides of the engine switch) on ONE shape - the longest - and one ragged size (257; t = 3 also
32769) on the others; the last case of every test repeats one size with every buffer at a multiple of 256 bytes (the control layout).
The 2-to-1 shapes (hash (2, 1), tree, forest, path verifier) need a rate of at least 2 and are left out at t = 2.
(A squeeze of out_len = 0 is not an empty call - an absorbing sponge is permuted, mod.rs:330-336 - and is not among the empty calls.)"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sponge_amd as S
from sponge_amd import _lib, synth
from oracle import cref
from oracle import poseidon_oracle as O

import arena

pytestmark = pytest.mark.gpu

FIELD = {"bls": (S.BLS12_381_FR, O.BLS12_381_FR, 255), "bn254": (S.BN254_FR, O.BN254_FR, 254)}
# label: (field, rate, alpha, RF, RP)
CONFIGS = {
    "t3": ("bls", 2, 5, 8, 31),
    "t4": ("bls", 3, 5, 8, 56),
    "t6": ("bls", 5, 5, 8, 57),
    "t9-bn254": ("bn254", 8, 5, 8, 57),
    "t9-alpha17": ("bls", 8, 17, 8, 57),
    "lds-t2": ("bls", 1, 5, 8, 31),
    "lds-t16": ("bls", 15, 5, 4, 6),
}
ENGINE = {"t4": b"HybridEngine<4,5", "t6": b"HybridEngine<6,5", "t9-bn254": b"HybridEngine<9,5", "t9-alpha17": b"HybridEngine<9,0",
          "lds-t2": b"LdsEngine<5>", "lds-t16": b"LdsEngine<5>"}
QUAD_MAX = 32768
ALL = list(CONFIGS)
RATE2 = [c for c in ALL if CONFIGS[c][1] >= 2]
ONCE = ["t3", "t9-bn254"]            # the once-per-entry-point checks: one t = 3 and one t = 9 config
E = 32


@functools.lru_cache(maxsize=None)
def _config(label):
    field, rate, alpha, rf, rp = CONFIGS[label]
    f, p, bits = FIELD[field]
    return f, S.poseidon_config_from_lfsr(f, rate, alpha, rf, rp), cref.CRef(O.make_config(p, bits, rate, alpha, rf, rp))


def _expected_engine(label, units):
    if label == "t3":
        return b"QuadEngine" if units <= QUAD_MAX else b"HybridEngine<3,5"
    return ENGINE[label]


def _cell(label, units):
    return label if label != "t3" else ("quad-t3" if units <= QUAD_MAX else "window-t3")


def _engine(entry, label, op, units, length=0):
    """the engine of one launch, asserted against the table; the span condition the guard width rests on"""
    f, cfg, cr = _config(label)
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(cfg.context()._h, op, units, length, ctypes.byref(info)))
    want = _expected_engine(label, units)
    assert info.engine.startswith(want), (entry, label, units, info.engine, want)
    if want.startswith(b"HybridEngine") and op in (_lib.OP_ABSORB, _lib.OP_SQUEEZE):
        assert b"passes" in info.engine
    assert info.width == cfg.t and arena.span_fits(info.threads, cfg.t), (info.threads, cfg.t, arena.G)
    print(f"{entry} [{label}] units={units} len={length}: {info.engine.decode()} ({info.threads} threads)")
    return info


def _sizes(label, full):
    """all batch sizes on the one full shape of an entry point, one ragged size on the others"""
    if full:
        return [1, 63, 65, 257, 1000] + ([32768, 32769] if label == "t3" else [])
    return [257] + ([32769] if label == "t3" else [])


def _stream():
    return torch.cuda.current_stream().cuda_stream


class DeviceArena:
    """the buffers of one call in one device allocation: fill on the host, one upload, a clone to compare with"""

    def __init__(self, buffers, seed, control=False):
        self.plan = arena.plan(buffers, control=control)
        self.image = self.plan.poisoned(seed)

    def put(self, name, data, at=None):
        self.plan.put(self.image, name, data, at)

    def upload(self):
        self.dev = torch.from_numpy(self.image).to("cuda:0")
        arena.assert_base_aligned(self.dev.data_ptr())
        self.before = self.dev.clone()
        torch.cuda.synchronize()
        if not self.plan.control:      # the residues hold for the real addresses
            for r in self.plan.regions:
                if r.align < 32:
                    assert self.ptr(r.name) % (2 * r.align) == r.align, (r.name, hex(self.ptr(r.name)))
        return self

    def ptr(self, name, shift=0):
        return self.plan.address(self.dev.data_ptr(), name, shift)

    def finish(self, written=None):
        torch.cuda.synchronize()
        self.plan.check(self.before, self.dev, written)

    def unchanged(self):
        torch.cuda.synchronize()
        assert torch.equal(self.before, self.dev), "the call changed the arena"

    def get(self, name, dtype=np.uint64):
        return self.plan.get(self.dev, name, dtype)


def _invoke(entry, label, a, shape, shift=None):
    """one *_dev call on the buffers of arena `a`; shift: {buffer: bytes} moves a pointer off its place.  Returns the status."""
    shift = shift or {}
    h, L, s = _config(label)[1].context()._h, _lib.lib(), _stream()

    def p(name):
        return a.ptr(name, shift.get(name, 0))
    if entry == "pmx_permute_batch_dev":
        return L.pmx_permute_batch_dev(h, p("d_states"), shape["n"], s)
    if entry == "pmx_hash_batch_dev":
        return L.pmx_hash_batch_dev(h, p("d_in"), shape["in_len"], p("d_out"), shape["out_len"], shape["n"], s)
    if entry == "pmx_sponge_absorb_batch_dev":
        return L.pmx_sponge_absorb_batch_dev(h, p("d_states"), p("d_mode_tag"), p("d_mode_index"), p("d_in"), shape["in_len"], shape["n"], s)
    if entry == "pmx_sponge_squeeze_batch_dev":
        return L.pmx_sponge_squeeze_batch_dev(h, p("d_states"), p("d_mode_tag"), p("d_mode_index"), p("d_out"), shape["out_len"], shape["n"], s)
    if entry == "pmx_sponge_absorb_varlen_batch_dev":
        return L.pmx_sponge_absorb_varlen_batch_dev(h, p("d_states"), p("d_mode_tag"), p("d_mode_index"), p("d_in"), p("d_offsets"),
                                                    shape["max_len"], shape["n"], s)
    if entry == "pmx_hash_varlen_batch_dev":
        return L.pmx_hash_varlen_batch_dev(h, p("d_in"), p("d_offsets"), shape["max_len"], p("d_out"), shape["out_len"], shape["n"], s)
    if entry == "pmx_merkle_2to1_dev":
        return L.pmx_merkle_2to1_dev(h, p("d_nodes"), shape["n_leaves"], s)
    if entry == "pmx_merkle_2to1_forest_dev":
        return L.pmx_merkle_2to1_forest_dev(h, p("d_nodes"), shape["n_trees"], shape["leaves_per_tree"], s)
    if entry == "pmx_merkle_verify_paths_dev":
        return L.pmx_merkle_verify_paths_dev(h, p("d_leaves"), p("d_indices"), p("d_paths"), shape["depth"], shape["k"], p("d_root"),
                                             p("d_ok"), p("d_work"), s)
    raise KeyError(entry)


def _ok(entry, label, a, shape):
    _lib.check(_invoke(entry, label, a, shape))


def _with_control(cases):
    """every case on the carved layout, then the second one again on the control layout"""
    return [(c, False) for c in cases] + [(cases[min(1, len(cases) - 1)], True)]


# ---- inputs and what the C port makes of them ------------------------------------------------------------------------------
def _modes(n, r, rng):
    """mixed tags, indices 0 .. r"""
    return rng.integers(0, 2, n).astype(np.uint32), rng.integers(0, r + 1, n).astype(np.uint32)


def _oracle_absorb(cr, st, tag, idx, rows):
    want_st, want_tag, want_idx = st.copy(), tag.copy(), idx.copy()
    for i, row in enumerate(rows):
        if len(row):     # an empty row leaves the sponge untouched (mod.rs:234-236)
            want_st[i], want_tag[i], want_idx[i] = cr.sponge_absorb(st[i], int(tag[i]), int(idx[i]), row)
    return want_st, want_tag, want_idx


def _oracle_squeeze(cr, st, tag, idx, out_len):
    want_st, want_tag, want_idx = st.copy(), tag.copy(), idx.copy()
    out = np.zeros((len(tag), out_len, 4), dtype=np.uint64)
    for i in range(len(tag)):
        want_st[i], want_tag[i], want_idx[i], out[i] = cr.sponge_squeeze(st[i], int(tag[i]), int(idx[i]), out_len)
    return want_st, want_tag, want_idx, out


def _sponges(f, t, r, n, seed):
    rng = np.random.default_rng(seed)
    st = synth.random_elements(f, n * t, seed=seed + 1).reshape(n, t, 4)
    tag, idx = _modes(n, r, rng)
    return st, tag, idx


def _put_sponges(a, st, tag, idx):
    a.put("d_states", st)
    a.put("d_mode_tag", tag)
    a.put("d_mode_index", idx)


def _assert_sponges(a, want, n, t, what):
    assert np.array_equal(a.get("d_states").reshape(n, t, 4), want[0]), what
    assert np.array_equal(a.get("d_mode_tag", np.uint32), want[1]), what
    assert np.array_equal(a.get("d_mode_index", np.uint32), want[2]), what


def _ragged(f, n, r, seed, skip=11):
    """lengths 0, 1, r - 1, r, r + 1, 2 r and random ones up to 5 r (the first row is never empty, so max_len > 0 at n = 1); the rows start
    behind `skip` other elements of the buffer (offsets[0] > 0)"""
    rng = np.random.default_rng(seed)
    base = [r + 1, 0, 1, max(r - 1, 0), r, 2 * r]
    lens = rng.integers(0, 5 * r + 1, n)
    k = min(n, 4 * len(base))
    lens[:k] = np.tile(base, 4)[:k]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[0] = skip
    offsets[1:] = np.cumsum(lens) + skip
    elems = np.ascontiguousarray(synth.random_elements(f, int(offsets[-1]) + 1, seed=seed + 2)[:int(offsets[-1])])
    rows = [elems[int(offsets[i]):int(offsets[i + 1])] for i in range(n)]
    return lens, offsets, elems, rows


# ---- the entry points --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ALL)
def test_permute_batch_dev(label):
    f, cfg, cr = _config(label)
    t = cfg.t
    for n, control in _with_control(_sizes(label, True)):
        _engine("pmx_permute_batch_dev", label, _lib.OP_PERMUTE, n)
        states = synth.random_elements(f, n * t, seed=1000 + n).reshape(n, t, 4)
        a = DeviceArena(arena.permute_buffers(t, n), seed=n, control=control)
        a.put("d_states", states)
        a.upload()
        _ok("pmx_permute_batch_dev", label, a, {"n": n})
        a.finish()
        assert np.array_equal(a.get("d_states").reshape(n, t, 4), cr.permute_batch(states, threads=0)), (label, n, control)


def _hash_shapes(label):
    r = CONFIGS[label][1]
    shapes = [((r + 2, r + 1), True), ((0, 1), False)]
    if r >= 2:
        shapes.append(((2, 1), False))        # the 2-to-1 launcher
    return shapes


def _hash_op(label, in_len, out_len):
    return _lib.OP_COMPRESS if (in_len, out_len) == (2, 1) and CONFIGS[label][1] >= 2 else _lib.OP_HASH


@pytest.mark.parametrize("label", ALL)
def test_hash_batch_dev(label):
    f, cfg, cr = _config(label)
    t = cfg.t
    for (in_len, out_len), full in _hash_shapes(label):
        for n, control in _with_control(_sizes(label, full)):
            _engine("pmx_hash_batch_dev", label, _hash_op(label, in_len, out_len), n, in_len)
            msgs = synth.random_elements(f, n * in_len + 1, seed=2000 + n)[:n * in_len].reshape(n, in_len, 4)
            a = DeviceArena(arena.hash_buffers(t, n, in_len, out_len), seed=n + in_len, control=control)
            a.put("d_in", msgs)
            a.upload()
            _ok("pmx_hash_batch_dev", label, a, {"n": n, "in_len": in_len, "out_len": out_len})
            a.finish()
            assert np.array_equal(a.get("d_out").reshape(n, out_len, 4), cr.hash_batch(msgs, in_len, out_len, threads=0)), \
                (label, n, in_len, out_len, control)


def _absorb_shapes(label):
    r = CONFIGS[label][1]
    return [(r + 1, True), (1, False)]


@pytest.mark.parametrize("label", ALL)
def test_sponge_absorb_batch_dev(label):
    f, cfg, cr = _config(label)
    t, r = cfg.t, cfg.rate
    for in_len, full in _absorb_shapes(label):
        for n, control in _with_control(_sizes(label, full)):
            _engine("pmx_sponge_absorb_batch_dev", label, _lib.OP_ABSORB, n, in_len)
            st, tag, idx = _sponges(f, t, r, n, seed=3000 + n + in_len)
            msgs = synth.random_elements(f, n * in_len, seed=3500 + n).reshape(n, in_len, 4)
            a = DeviceArena(arena.absorb_buffers(t, n, in_len), seed=n + in_len, control=control)
            _put_sponges(a, st, tag, idx)
            a.put("d_in", msgs)
            a.upload()
            _ok("pmx_sponge_absorb_batch_dev", label, a, {"n": n, "in_len": in_len})
            a.finish()
            _assert_sponges(a, _oracle_absorb(cr, st, tag, idx, msgs), n, t, (label, n, in_len, control))


def _squeeze_shapes(label):
    r = CONFIGS[label][1]
    return [(2 * r + 1, True), (1, False), (r, False)]


@pytest.mark.parametrize("label", ALL)
def test_sponge_squeeze_batch_dev(label):
    """(the window engines copy the squeezed elements out of the wave's LDS staging: copy_out_staged)"""
    f, cfg, cr = _config(label)
    t, r = cfg.t, cfg.rate
    for out_len, full in _squeeze_shapes(label):
        for n, control in _with_control(_sizes(label, full)):
            _engine("pmx_sponge_squeeze_batch_dev", label, _lib.OP_SQUEEZE, n, out_len)
            st, tag, idx = _sponges(f, t, r, n, seed=4000 + n + out_len)
            a = DeviceArena(arena.squeeze_buffers(t, n, out_len), seed=n + out_len, control=control)
            _put_sponges(a, st, tag, idx)
            a.upload()
            _ok("pmx_sponge_squeeze_batch_dev", label, a, {"n": n, "out_len": out_len})
            a.finish()
            want = _oracle_squeeze(cr, st, tag, idx, out_len)
            _assert_sponges(a, want, n, t, (label, n, out_len, control))
            assert np.array_equal(a.get("d_out").reshape(n, out_len, 4), want[3]), (label, n, out_len, control)


@pytest.mark.parametrize("label", ALL)
def test_sponge_absorb_varlen_batch_dev(label):
    f, cfg, cr = _config(label)
    t, r = cfg.t, cfg.rate
    for n, control in _with_control(_sizes(label, True)):
        lens, offsets, elems, rows = _ragged(f, n, r, seed=5000 + n)
        max_len = int(lens.max())          # equal to the longest row
        _engine("pmx_sponge_absorb_varlen_batch_dev", label, _lib.OP_ABSORB, n, max_len)
        st, tag, idx = _sponges(f, t, r, n, seed=5500 + n)
        if n >= 24:      # empty rows (1, 7, 13) on the sponges a non-empty absorb would permute first
            tag[[1, 7, 13]] = [S.MODE_SQUEEZING, S.MODE_ABSORBING, S.MODE_SQUEEZING]
            idx[[1, 7, 13]] = [r, r, 0]
        a = DeviceArena(arena.absorb_varlen_buffers(t, n, elems.shape[0]), seed=n, control=control)
        _put_sponges(a, st, tag, idx)
        a.put("d_in", elems)
        a.put("d_offsets", offsets)
        a.upload()
        _ok("pmx_sponge_absorb_varlen_batch_dev", label, a, {"n": n, "max_len": max_len})
        a.finish()
        _assert_sponges(a, _oracle_absorb(cr, st, tag, idx, rows), n, t, (label, n, control))


def _hash_varlen_shapes(label):
    r = CONFIGS[label][1]
    return [(r + 1, True), (1, False)]


@pytest.mark.parametrize("label", ALL)
def test_hash_varlen_batch_dev(label):
    f, cfg, cr = _config(label)
    t, r = cfg.t, cfg.rate
    for out_len, full in _hash_varlen_shapes(label):
        for n, control in _with_control(_sizes(label, full)):
            lens, offsets, elems, rows = _ragged(f, n, r, seed=6000 + n + out_len)
            max_len = int(lens.max())
            _engine("pmx_hash_varlen_batch_dev", label, _lib.OP_ABSORB, n, max_len)
            _engine("pmx_hash_varlen_batch_dev", label, _lib.OP_SQUEEZE, n, out_len)
            a = DeviceArena(arena.hash_varlen_buffers(t, n, elems.shape[0], out_len), seed=n + out_len, control=control)
            a.put("d_in", elems)
            a.put("d_offsets", offsets)
            a.upload()
            _ok("pmx_hash_varlen_batch_dev", label, a, {"n": n, "max_len": max_len, "out_len": out_len})
            a.finish()
            got = a.get("d_out").reshape(n, out_len, 4)
            for length in np.unique(lens):
                which = np.nonzero(lens == length)[0]
                msgs = np.stack([rows[i] for i in which]).reshape(len(which), int(length), 4)
                assert np.array_equal(got[which], cr.hash_batch(msgs, int(length), out_len, threads=0)), (label, n, out_len, int(length), control)


def _tree_sizes(label):
    return [2, 64, 4096] + ([1 << 17] if label == "t3" else [])      # 2^17: level 1 is 65536 compressions, across the 32768 switch


@pytest.mark.parametrize("label", RATE2)
def test_merkle_2to1_dev(label):
    f, cfg, cr = _config(label)
    for m, control in _with_control(_tree_sizes(label)):
        for width in sorted({m // 2, 1}):
            _engine("pmx_merkle_2to1_dev", label, _lib.OP_COMPRESS, width)
        leaves = synth.random_elements(f, m, seed=7000 + m)
        a = DeviceArena(arena.merkle_buffers(cfg.t, m), seed=m, control=control)
        a.put("d_nodes", leaves, at=0)
        a.upload()
        _ok("pmx_merkle_2to1_dev", label, a, {"n_leaves": m})
        a.finish(written=arena.merkle_written(m))          # the leaves rows count as `in`
        assert np.array_equal(a.get("d_nodes").reshape(2 * m - 1, 4), cr.merkle(leaves, threads=0)), (label, m, control)


FORESTS = [(3, 16), (5, 1), (40000, 2)]


def _oracle_forest(cr, leaves, n_trees, m):
    """level-major: all leaves, then level 1 of every tree (tree after tree), ..., the roots.  Tree b's node j of level l is row
    n_trees * (2 m - 2 m / 2^l) + b * (m / 2^l) + j (include/poseidon_mi355x.h); small forests are placed tree by tree from the C port's
    own trees, a wide one level by level (its levels are the C port's batch hash over the pairs, which never straddle two trees)."""
    nodes = np.zeros((n_trees * (2 * m - 1), 4), dtype=np.uint64)
    if n_trees <= 8:
        for b in range(n_trees):
            tree = cr.merkle(leaves[b * m:(b + 1) * m]) if m > 1 else leaves[b:b + 1]
            first, level = 0, 0
            while (m >> level) >= 1:
                w = m >> level
                row = n_trees * (2 * m - 2 * m // (1 << level)) + b * w
                nodes[row:row + w] = tree[first:first + w]
                first, level = first + w, level + 1
        return nodes
    nodes[:n_trees * m] = leaves
    src, width = 0, n_trees * m
    while width > n_trees:
        nodes[src + width:src + width + width // 2] = cr.hash_batch(nodes[src:src + width].reshape(width // 2, 2, 4), 2, 1, threads=0).reshape(-1, 4)
        src, width = src + width, width // 2
    return nodes


@pytest.mark.parametrize("label", RATE2)
def test_merkle_2to1_forest_dev(label):
    f, cfg, cr = _config(label)
    for (n_trees, m), control in _with_control(FORESTS):
        if m > 1:
            for width in sorted({n_trees * m // 2, n_trees}):
                _engine("pmx_merkle_2to1_forest_dev", label, _lib.OP_COMPRESS, width)
        leaves = synth.random_elements(f, n_trees * m, seed=8000 + n_trees)
        a = DeviceArena(arena.forest_buffers(cfg.t, n_trees, m), seed=n_trees, control=control)
        a.put("d_nodes", leaves, at=0)
        a.upload()
        _ok("pmx_merkle_2to1_forest_dev", label, a, {"n_trees": n_trees, "leaves_per_tree": m})
        a.finish(written=arena.forest_written(n_trees, m))
        assert np.array_equal(a.get("d_nodes").reshape(-1, 4), _oracle_forest(cr, leaves, n_trees, m)), (label, n_trees, m, control)


DEPTH = 6


def _path_counts(label):
    return [1, 65, 1000] + ([QUAD_MAX + 65] if label == "t3" else [])      # (t = 3: the level steps of that many paths run on the window engine)


def _paths(f, cr, k, seed):
    """k authentication paths over a 64-leaf tree - good ones, a flipped sibling, a foreign leaf, an index with a bit above the depth -
    and what the C port says of each: hash the leaf up its path, compare with the root, index < 2^depth"""
    rng = np.random.default_rng(seed)
    m = 1 << DEPTH
    tree_leaves = synth.random_elements(f, m, seed=seed)
    nodes = cr.merkle(tree_leaves, threads=0)
    indices = rng.integers(0, m, k).astype(np.uint64)
    leaves = tree_leaves[indices.astype(np.int64)].copy()
    paths = np.zeros((k, DEPTH, 4), dtype=np.uint64)
    pos, first, width = indices.astype(np.int64), 0, m
    for level in range(DEPTH):
        paths[:, level] = nodes[first + (pos ^ 1)]
        first, width, pos = first + width, width // 2, pos >> 1
    kind = rng.integers(0, 4, k) if k > 1 else np.zeros(1, dtype=np.int64)     # 0: good
    kind[:min(k, 4)] = [0, 1, 2, 3][:min(k, 4)]
    bad = np.nonzero(kind == 1)[0]
    paths[bad, rng.integers(0, DEPTH, len(bad)), rng.integers(0, 4, len(bad))] ^= np.uint64(1)
    foreign = np.nonzero(kind == 2)[0]
    leaves[foreign] = synth.random_elements(f, len(foreign) + 1, seed=seed + 1)[:len(foreign)]
    high = np.nonzero(kind == 3)[0]
    indices[high] += np.uint64(m)          # the low bits still walk a good path: only the range test can fail it
    cur = leaves.copy()
    for level in range(DEPTH):
        right = ((indices >> np.uint64(level)) & np.uint64(1)).astype(bool)
        pairs = np.where(right[:, None, None], np.stack([paths[:, level], cur], axis=1), np.stack([cur, paths[:, level]], axis=1))
        cur = cr.hash_batch(pairs, 2, 1, threads=0).reshape(k, 4)
    ok = ((cur == nodes[-1]).all(axis=1) & (indices < m)).astype(np.uint8)
    assert np.array_equal(ok, (kind == 0).astype(np.uint8))
    return leaves, indices, paths, nodes[-1].copy(), ok


@pytest.mark.parametrize("label", RATE2)
def test_merkle_verify_paths_dev(label):
    """d_ok is k single bytes at an odd address; d_work is scratch (may be written, not compared)"""
    f, cfg, cr = _config(label)
    for k, control in _with_control(_path_counts(label)):
        _engine("pmx_merkle_verify_paths_dev", label, _lib.OP_COMPRESS, k)
        leaves, indices, paths, root, ok = _paths(f, cr, k, seed=9000 + k)
        a = DeviceArena(arena.verify_paths_buffers(cfg.t, DEPTH, k), seed=k, control=control)
        for name, data in (("d_leaves", leaves), ("d_indices", indices), ("d_paths", paths), ("d_root", root)):
            a.put(name, data)
        a.upload()
        if not control:
            assert a.ptr("d_ok") % 2 == 1
        _ok("pmx_merkle_verify_paths_dev", label, a, {"depth": DEPTH, "k": k})
        a.finish()
        got = a.get("d_ok", np.uint8)
        assert np.array_equal(got, ok), (label, k, control)
        assert k < 4 or (got.min(), got.max()) == (0, 1)      # both values occur


def test_no_engine_x_entry_point_cell_is_empty():
    """the case tables above, asked of pmx_ctx_engine_info: every entry point runs on every engine that serves it"""
    cells = set()

    def add(entry, label, op, units, length=0):
        info = _lib.PmxEngineInfo()
        _lib.check(_lib.lib().pmx_ctx_engine_info(_config(label)[1].context()._h, op, units, length, ctypes.byref(info)))
        assert info.engine.startswith(_expected_engine(label, units))
        cells.add((entry, _cell(label, units)))
    for label in ALL:
        r = CONFIGS[label][1]
        for n in _sizes(label, True):
            add("permute", label, _lib.OP_PERMUTE, n)
            add("absorb_varlen", label, _lib.OP_ABSORB, n, 5 * r)
        for (in_len, out_len), full in _hash_shapes(label):
            for n in _sizes(label, full):
                add(f"hash ({'r + 2, r + 1' if in_len > 2 else f'{in_len}, {out_len}'})", label, _hash_op(label, in_len, out_len), n, in_len)
        for shapes, entry, op in ((_absorb_shapes, "absorb", _lib.OP_ABSORB), (_squeeze_shapes, "squeeze", _lib.OP_SQUEEZE),
                                  (_hash_varlen_shapes, "hash_varlen", _lib.OP_SQUEEZE)):
            for length, full in shapes(label):
                for n in _sizes(label, full):
                    add(entry, label, op, n, length)
        if r >= 2:
            for m in _tree_sizes(label):
                add("merkle", label, _lib.OP_COMPRESS, m // 2)
            for n_trees, m in FORESTS:
                if m > 1:
                    add("forest", label, _lib.OP_COMPRESS, n_trees * m // 2)
            for k in _path_counts(label):
                add("verify_paths", label, _lib.OP_COMPRESS, k)
    engines = ["quad-t3", "window-t3", "t4", "t6", "t9-bn254", "t9-alpha17", "lds-t2", "lds-t16"]
    every = ["permute", "hash (0, 1)", "hash (r + 2, r + 1)", "absorb", "squeeze", "absorb_varlen", "hash_varlen"]
    two_to_one = ["hash (2, 1)", "merkle", "forest", "verify_paths"]
    want = {(e, g) for e in every for g in engines} | {(e, g) for e in two_to_one for g in engines if g != "lds-t2"}
    assert cells == want, (sorted(want - cells), sorted(cells - want))


# ---- once per entry point, on one t = 3 and one t = 9 config -------------------------------------------------------------------
N_ONCE = 65


def _laid_out(entry, label, seed=77):
    """a valid call of N_ONCE units in an arena: (arena, shape, buffers pmx_host_call.cpp checks with aligned16)"""
    f, cfg, cr = _config(label)
    t, r, n = cfg.t, cfg.rate, N_ONCE
    st, tag, idx = _sponges(f, t, r, n, seed)
    lens, offsets, elems, rows = _ragged(f, n, r, seed)
    if entry == "pmx_permute_batch_dev":
        a, shape, checked = DeviceArena(arena.permute_buffers(t, n), seed), {"n": n}, ["d_states"]
        a.put("d_states", st)
    elif entry == "pmx_hash_batch_dev":
        a, shape, checked = DeviceArena(arena.hash_buffers(t, n, r + 2, r + 1), seed), {"n": n, "in_len": r + 2, "out_len": r + 1}, ["d_in", "d_out"]
        a.put("d_in", synth.random_elements(f, n * (r + 2), seed=seed))
    elif entry == "pmx_sponge_absorb_batch_dev":
        a, shape, checked = DeviceArena(arena.absorb_buffers(t, n, r + 1), seed), {"n": n, "in_len": r + 1}, ["d_states", "d_in"]
        _put_sponges(a, st, tag, idx)
        a.put("d_in", synth.random_elements(f, n * (r + 1), seed=seed))
    elif entry == "pmx_sponge_squeeze_batch_dev":
        a, shape, checked = DeviceArena(arena.squeeze_buffers(t, n, 2 * r + 1), seed), {"n": n, "out_len": 2 * r + 1}, ["d_states", "d_out"]
        _put_sponges(a, st, tag, idx)
    elif entry == "pmx_sponge_absorb_varlen_batch_dev":
        a, shape, checked = DeviceArena(arena.absorb_varlen_buffers(t, n, elems.shape[0]), seed), {"n": n, "max_len": int(lens.max())}, ["d_states", "d_in"]
        _put_sponges(a, st, tag, idx)
        a.put("d_in", elems)
        a.put("d_offsets", offsets)
    elif entry == "pmx_hash_varlen_batch_dev":
        a = DeviceArena(arena.hash_varlen_buffers(t, n, elems.shape[0], r + 1), seed)
        shape, checked = {"n": n, "max_len": int(lens.max()), "out_len": r + 1}, ["d_in", "d_out"]
        a.put("d_in", elems)
        a.put("d_offsets", offsets)
    elif entry == "pmx_merkle_2to1_dev":
        a, shape, checked = DeviceArena(arena.merkle_buffers(t, 64), seed), {"n_leaves": 64}, ["d_nodes"]
        a.put("d_nodes", synth.random_elements(f, 64, seed=seed), at=0)
    elif entry == "pmx_merkle_2to1_forest_dev":
        a, shape, checked = DeviceArena(arena.forest_buffers(t, 3, 16), seed), {"n_trees": 3, "leaves_per_tree": 16}, ["d_nodes"]
        a.put("d_nodes", synth.random_elements(f, 48, seed=seed), at=0)
    else:
        a, shape = DeviceArena(arena.verify_paths_buffers(t, DEPTH, n), seed), {"depth": DEPTH, "k": n}
        checked = ["d_leaves", "d_paths", "d_work", "d_root"]
        leaves, indices, paths, root, ok = _paths(f, cr, n, seed)
        for name, data in (("d_leaves", leaves), ("d_indices", indices), ("d_paths", paths), ("d_root", root)):
            a.put(name, data)
    return a.upload(), shape, checked


ENTRIES = ["pmx_permute_batch_dev", "pmx_hash_batch_dev", "pmx_sponge_absorb_batch_dev", "pmx_sponge_squeeze_batch_dev",
           "pmx_sponge_absorb_varlen_batch_dev", "pmx_hash_varlen_batch_dev", "pmx_merkle_2to1_dev", "pmx_merkle_2to1_forest_dev",
           "pmx_merkle_verify_paths_dev"]
# the empty forms of a call: shape entries that replace those of the valid call
EMPTY = {
    "pmx_permute_batch_dev": [{"n": 0}],
    "pmx_hash_batch_dev": [{"n": 0}],
    "pmx_sponge_absorb_batch_dev": [{"n": 0}, {"in_len": 0}],                 # absorbing an empty input changes nothing (mod.rs:234-236)
    "pmx_sponge_squeeze_batch_dev": [{"n": 0}],
    "pmx_sponge_absorb_varlen_batch_dev": [{"n": 0}, {"max_len": 0}],         # every row clamped to empty
    "pmx_hash_varlen_batch_dev": [{"n": 0}, {"out_len": 0}],                  # nothing to write
    "pmx_merkle_2to1_dev": [{"n_leaves": 1}],                                 # a tree of one leaf is its own root: no level to write
    "pmx_merkle_2to1_forest_dev": [{"leaves_per_tree": 1}],
    "pmx_merkle_verify_paths_dev": [{"k": 0}],
}


@pytest.mark.parametrize("label", ONCE)
@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_calls_return_ok_and_touch_nothing(entry, label):
    a, shape, _ = _laid_out(entry, label)
    for empty in EMPTY[entry]:
        assert _invoke(entry, label, a, {**shape, **empty}) == _lib.PMX_OK, (entry, empty, _lib.lib().pmx_last_error())
        a.unchanged()


@pytest.mark.parametrize("label", ONCE)
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_pointer_at_8_mod_16_is_refused(entry, label):
    f, cfg, cr = _config(label)
    a, shape, checked = _laid_out(entry, label)
    for name in checked:
        assert a.ptr(name, 8) % 16 == 8
        assert _invoke(entry, label, a, shape, shift={name: 8}) == _lib.PMX_ERR_ARG, (entry, name)
        assert b"16-byte aligned" in _lib.lib().pmx_last_error(), (entry, name, _lib.lib().pmx_last_error())
        a.unchanged()
    # the context still computes a correct permutation
    states = synth.random_elements(f, N_ONCE * cfg.t, seed=5).reshape(N_ONCE, cfg.t, 4)
    assert np.array_equal(cfg.context().permute_batch(states), cr.permute_batch(states, threads=0))


# ---- the host entry points on a view into a larger host array ------------------------------------------------------------------
def _host_image(p, seed, pinned):
    """a poisoned host image of plan p whose base is 256-byte aligned: pageable (numpy) or page-locked (pmx_host_alloc)"""
    if pinned:
        image = S.pinned_empty((p.size + 7) // 8).view(np.uint8)[:p.size]
    else:
        raw = np.empty(p.size + 256, dtype=np.uint8)
        image = raw[(-raw.ctypes.data) % 256:][:p.size]
    arena.assert_base_aligned(image.ctypes.data)
    image[:] = p.poisoned(seed)
    return image


# pageable: the view starts at 8 mod 16; (1 << 18) + 5 rows are more than the 16 MiB that are page-locked for the length of the call, at an
# address that is not page-aligned.  page-locked: the view starts 16 bytes into the allocation's layout (16 mod 32).
HOST = [("pageable", 100), ("pageable", (1 << 18) + 5), ("pinned", (1 << 16) + 77)]


@pytest.mark.parametrize("label", ONCE)
@pytest.mark.parametrize("memory,n", HOST)
def test_host_permute_on_a_view_into_a_larger_array(memory, n, label):
    f, cfg, cr = _config(label)
    t = cfg.t
    align = 8 if memory == "pageable" else 16
    p = arena.plan([("states", n * t * E, align, "inout")])
    image = _host_image(p, n, memory == "pinned")
    states = synth.random_elements(f, n * t, seed=n).reshape(n, t, 4)
    p.put(image, "states", states)
    address = p.address(image.ctypes.data, "states")
    assert address % (2 * align) == align and (memory == "pinned" or address % 4096 != 0)
    before = image.copy()
    _lib.check(_lib.lib().pmx_permute_batch(cfg.context()._h, address, n))
    p.check(before, image)                                # the host guards
    assert np.array_equal(p.get(image, "states").reshape(n, t, 4), cr.permute_batch(states, threads=0)), (memory, n)


@pytest.mark.parametrize("label", ONCE)
@pytest.mark.parametrize("memory,n", HOST)
def test_host_hash_on_a_view_into_a_larger_array(memory, n, label):
    """(t = 9: one digest element per row keeps the C port's share of the large case in hand - the input alone is above 16 MiB)"""
    f, cfg, cr = _config(label)
    r = cfg.rate
    in_len, out_len = r + 2, (r + 1 if label == "t3" else 1)
    align = 8 if memory == "pageable" else 16
    p = arena.plan([("in", n * in_len * E, align, "in"), ("out", n * out_len * E, align, "out")])
    image = _host_image(p, n + 1, memory == "pinned")
    msgs = synth.random_elements(f, n * in_len, seed=n + 1).reshape(n, in_len, 4)
    p.put(image, "in", msgs)
    for name in ("in", "out"):
        assert p.address(image.ctypes.data, name) % (2 * align) == align
    before = image.copy()
    _lib.check(_lib.lib().pmx_hash_batch(cfg.context()._h, p.address(image.ctypes.data, "in"), in_len,
                                         p.address(image.ctypes.data, "out"), out_len, n))
    p.check(before, image)                                # the host guards and the const input
    assert np.array_equal(p.get(image, "out").reshape(n, out_len, 4), cr.hash_batch(msgs, in_len, out_len, threads=0)), (memory, n)
