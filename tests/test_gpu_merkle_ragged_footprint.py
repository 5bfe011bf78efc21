"""The memory footprint of the four *_dev entry points of the trees over any number of leaves (pmx_merkle_ragged_dev,
pmx_merkle_ragged_paths_dev, pmx_merkle_ragged_verify_paths_dev, pmx_merkle_ragged_update_dev), as tests/test_gpu_merkle_ary_footprint.py
does it for the arity-k entries: all buffers of a call carved out of ONE poisoned device allocation at the documented alignment and
nothing above it, 256 KiB of guard around each (tests/arena.py).  After the call every out buffer equals the oracle in full and every
byte outside d_nodes[0 .. n_nodes), the paths, d_ok and d_work is unchanged - so a short parent that stored or (through the oracle's
digest) loaded beyond its level shows.

One window-engine case (BN254 t = 9, arity 8, 521 leaves: levels of 66, 9, 2, 1), one run-time-width case (t = 16, arity 15, 976 leaves:
66, 5, 1) and one quad-engine case (t = 3, arity 2, 131 leaves: 66, 33, 17, 9, 5, 3, 2, 1): the widest level is one full wave and two
lanes, its last parent has one child, and further levels are short too.  65 openings, paths and updates.  Every test runs on
the carved layout and again with every buffer at a multiple of 256 bytes (the control layout)."""
import ctypes

import numpy as np
import pytest
import torch

from sponge_amd import _lib, synth

import arena
import merkle_ary_oracle as MA
import merkle_ragged_oracle as M
from test_gpu_footprint import DeviceArena

pytestmark = pytest.mark.gpu

E = arena.E
CASES = [("t9-bn254", 8, 521, b"HybridEngine<9,5"), ("lds-t16", 15, 976, b"LdsEngine<5>"), ("t3", 2, 131, b"QuadEngine<5>")]
UNITS = 65
U64 = (1 << 64) - 1


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _h(label):
    return M.config(label)[1].context()._h


def _engine(label, a, want, units):
    """the engine of the level, asserted; the span condition the guard width rests on (tests/arena.py)"""
    info = _lib.PmxEngineInfo()
    cfg = M.config(label)[1]
    _lib.check(_lib.lib().pmx_ctx_engine_info(cfg.context()._h, _lib.OP_COMPRESS, units, a, ctypes.byref(info)))
    assert info.engine.startswith(want), (label, units, info.engine)
    assert info.width == cfg.t and arena.span_fits(info.threads, cfg.t)


def paths_buffers(n_nodes, depth, a, k):
    return [("d_nodes", n_nodes * E, 16, "in"), ("d_indices", k * 8, 8, "in"), ("d_paths", k * depth * (a - 1) * E, 16, "out")]


def verify_buffers(depth, a, k):
    return [("d_leaves", k * E, 16, "in"), ("d_indices", k * 8, 8, "in"), ("d_paths", k * depth * (a - 1) * E, 16, "in"), ("d_root", E, 16, "in"),
            ("d_ok", k, 1, "out"), ("d_work", k * (a + 1) * 4 * 8, 16, "scratch")]


def update_buffers(n_nodes, a, k):
    return [("d_nodes", n_nodes * E, 16, "inout"), ("d_indices", k * 8, 8, "in"), ("d_new_leaves", k * E, 16, "in"),
            ("d_work", k * (a + 1) * 4 * 8, 16, "scratch")]


@pytest.mark.parametrize("label,a,m,engine", CASES)
def test_merkle_ragged_dev(label, a, m, engine):
    leaves, want = M.cached_tree(label, a, m)
    w = M.widths(m, a)
    assert w[1] == UNITS + 1 and w[0] % a == 1 and sum(x % a != 0 for x in w[:-1]) >= 2
    for control in (False, True):
        for units in w[1:]:
            _engine(label, a, engine, units)
        ar = DeviceArena([("d_nodes", want.shape[0] * E, 16, "out")], seed=1, control=control)
        ar.put("d_nodes", leaves, at=0)
        ar.upload()
        _lib.check(_lib.lib().pmx_merkle_ragged_dev(_h(label), ar.ptr("d_nodes"), m, a, _stream()))
        ar.finish(written={"d_nodes": (m * E, want.shape[0] * E)})       # the leaves rows count as `in`
        assert np.array_equal(ar.get("d_nodes").reshape(-1, 4), want), (label, control)


def _path_case(label, a, m):
    """65 openings, good and bad ones, with the verdicts of the oracle's whole-row climb"""
    f, cfg, cr = M.config(label)
    leaves, nodes = M.cached_tree(label, a, m)
    depth = M.shape(m, a)[0]
    idx = M.path_indices(m, a, UNITS, seed=a)
    paths = M.open_paths(nodes, m, a, idx)
    bad = paths.copy()
    bad[1::2, 1, a - 2, 3] ^= np.uint64(2)                  # every second path: one limb of the last sibling of level 1, absent ones too
    vidx = idx.copy()
    mine = np.array(leaves[idx.astype(np.int64)])
    # path 4: slot m of the short bottom parent - a zero `leaf` whose row is that parent's: only the range test fails it
    vidx[4] = m
    mine[4] = 0
    bad[4] = M.open_paths(nodes, m, a, [m - 1])[0]
    bad[4, 0] = 0
    bad[4, 0, 0] = leaves[m - 1]
    top = MA.climb(cr, mine, vidx, bad, a)
    assert (top[4] == nodes[-1]).all(), "the forged path climbs to the root"
    ok = ((top == nodes[-1]).all(axis=1) & (vidx < np.uint64(m))).astype(np.uint8)
    assert ok[0] == 1 and ok[1] == 0 and ok[4] == 0 and 0 < ok.sum() < UNITS
    return depth, nodes, idx, paths, mine, vidx, bad, ok


@pytest.mark.parametrize("label,a,m,engine", CASES)
def test_merkle_ragged_paths_dev(label, a, m, engine):
    """only d_paths changes; d_indices sits at 8 mod 16"""
    depth, nodes, idx, paths, *_ = _path_case(label, a, m)
    idx = idx.copy()
    idx[7], idx[9] = m, U64                                 # indices that name no leaf: all-zero paths
    paths = paths.copy()
    paths[[7, 9]] = 0
    for control in (False, True):
        ar = DeviceArena(paths_buffers(nodes.shape[0], depth, a, UNITS), seed=7, control=control)
        ar.put("d_nodes", nodes)
        ar.put("d_indices", idx)
        ar.upload()
        _lib.check(_lib.lib().pmx_merkle_ragged_paths_dev(_h(label), ar.ptr("d_nodes"), m, a, ar.ptr("d_indices"), UNITS, ar.ptr("d_paths"),
                                                          _stream()))
        ar.finish()
        assert np.array_equal(ar.get("d_paths").reshape(paths.shape), paths), (label, control)


@pytest.mark.parametrize("label,a,m,engine", CASES)
def test_merkle_ragged_verify_paths_dev(label, a, m, engine):
    """d_ok is 65 single bytes at an odd address; d_work is scratch (may be written, not compared)"""
    depth, nodes, idx, paths, mine, vidx, bad, ok = _path_case(label, a, m)
    L, s = _lib.lib(), _stream()
    for control in (False, True):
        _engine(label, a, engine, UNITS)
        ar = DeviceArena(verify_buffers(depth, a, UNITS), seed=9, control=control)
        for name, data in (("d_leaves", mine), ("d_indices", vidx), ("d_paths", bad), ("d_root", np.array(nodes[-1]))):
            ar.put(name, data)
        ar.upload()
        if not control:
            assert ar.ptr("d_ok") % 2 == 1
            for name in ("d_leaves", "d_paths", "d_work", "d_root"):
                p = {n: ar.ptr(n, 8 if n == name else 0) for n in ("d_leaves", "d_indices", "d_paths", "d_root", "d_ok", "d_work")}
                rc = L.pmx_merkle_ragged_verify_paths_dev(_h(label), p["d_leaves"], p["d_indices"], p["d_paths"], depth, a, m, UNITS, p["d_root"],
                                                          p["d_ok"], p["d_work"], s)
                assert rc == _lib.PMX_ERR_ARG and b"16-byte aligned" in L.pmx_last_error(), (name, L.pmx_last_error())
                ar.unchanged()
        _lib.check(L.pmx_merkle_ragged_verify_paths_dev(_h(label), ar.ptr("d_leaves"), ar.ptr("d_indices"), ar.ptr("d_paths"), depth, a, m, UNITS,
                                                        ar.ptr("d_root"), ar.ptr("d_ok"), ar.ptr("d_work"), s))
        ar.finish()
        got = ar.get("d_ok", np.uint8)
        assert np.array_equal(got, ok), (label, control)
        assert (got.min(), got.max()) == (0, 1)


def _update_case(label, a, m, out_of_range):
    """(indices, new leaves, the oracle's old tree, its rebuild with the in-range updates applied): 65 distinct indices, the last leaf -
    the only child of its parent - among them"""
    f, cfg, cr = M.config(label)
    leaves, old = M.cached_tree(label, a, m)
    picks = list(dict.fromkeys([m - 1, 0] + [int(x) for x in np.random.default_rng(a).permutation(m)]))[:UNITS]
    idx = np.array(picks, dtype=np.uint64)
    new = synth.random_elements(f, UNITS, seed=600 + a)
    if out_of_range:
        idx[3], idx[17], idx[64] = m, U64, m + a - 2        # (m and m + a - 2: slots of the short bottom parent that hold no leaf)
    after = np.array(leaves, dtype=np.uint64)
    for i, j in enumerate(int(x) for x in idx):
        if j < m:
            after[j] = new[i]
    return idx, new, old, M.tree(cr, after, a)


@pytest.mark.parametrize("out_of_range", [False, True])
@pytest.mark.parametrize("label,a,m,engine", CASES)
def test_merkle_ragged_update_dev(label, a, m, engine, out_of_range):
    idx, new, old, want = _update_case(label, a, m, out_of_range)
    w = M.widths(m, a)
    assert w[1] > UNITS >= w[2], "gathered rows at the first level, whole levels above"
    L, s = _lib.lib(), _stream()
    for control in (False, True):
        ar = DeviceArena(update_buffers(old.shape[0], a, UNITS), seed=11, control=control)
        ar.put("d_nodes", old)
        ar.put("d_indices", idx)
        ar.put("d_new_leaves", new)
        ar.upload()
        if not control:
            assert ar.ptr("d_indices") % 16 == 8
            for name in ("d_nodes", "d_new_leaves", "d_work"):
                p = {n: ar.ptr(n, 8 if n == name else 0) for n in ("d_nodes", "d_indices", "d_new_leaves", "d_work")}
                rc = L.pmx_merkle_ragged_update_dev(_h(label), p["d_nodes"], m, a, p["d_indices"], p["d_new_leaves"], UNITS, p["d_work"], s)
                assert rc == _lib.PMX_ERR_ARG and b"16-byte aligned" in L.pmx_last_error(), (name, L.pmx_last_error())
                ar.unchanged()
        _lib.check(L.pmx_merkle_ragged_update_dev(_h(label), ar.ptr("d_nodes"), m, a, ar.ptr("d_indices"), ar.ptr("d_new_leaves"), UNITS,
                                                  ar.ptr("d_work"), s))
        ar.finish()
        assert np.array_equal(ar.get("d_nodes").reshape(-1, 4), want), (label, control, out_of_range)
