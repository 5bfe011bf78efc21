"""The memory footprint of the four *_dev entry points of the arity-k trees (pmx_merkle_ary_dev, pmx_merkle_ary_forest_dev,
pmx_merkle_ary_paths_dev, pmx_merkle_ary_verify_paths_dev), as tests/test_gpu_footprint.py does it for the 2-to-1 entries: all buffers
of a call carved out of ONE poisoned device allocation at the documented alignment and nothing above it, 256 KiB of guard around each
(tests/arena.py).  After the call every out buffer equals the oracle in full and every byte outside the documented arrays is unchanged.

One window-engine case (BN254 t = 9, arity 8) and one run-time-width case (t = 16, arity 15).  Units: 65 - one full wave and one lane -
for the forest (65 trees), the openings and the verifier (65 paths); a single tree cannot have 65 parents, so it takes the smallest
shape with more than one wave in its widest level (512 parents at arity 8, 225 at arity 15).  The last case of every test repeats the
call with every buffer at a multiple of 256 bytes (the control layout)."""
import ctypes

import numpy as np
import pytest
import torch

from sponge_amd import _lib, synth

import arena
import merkle_ary_oracle as M
from test_gpu_footprint import DeviceArena

pytestmark = pytest.mark.gpu

E = arena.E
CASES = [("t9-bn254", 8, b"HybridEngine<9,5"), ("lds-t16", 15, b"LdsEngine<5>")]
UNITS = 65


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ctx(label):
    return M.config(label)[1].context()


def _engine(label, a, want, units):
    """the engine of the level, asserted; the span condition the guard width rests on (tests/arena.py)"""
    info = _lib.PmxEngineInfo()
    cfg = M.config(label)[1]
    _lib.check(_lib.lib().pmx_ctx_engine_info(cfg.context()._h, _lib.OP_COMPRESS, units, a, ctypes.byref(info)))
    assert info.engine.startswith(want), (label, units, info.engine)
    assert info.width == cfg.t and arena.span_fits(info.threads, cfg.t)


def tree_buffers(n_nodes):
    return [("d_nodes", n_nodes * E, 16, "out")]


def paths_buffers(n_nodes, depth, a, k):
    return [("d_nodes", n_nodes * E, 16, "in"), ("d_indices", k * 8, 8, "in"), ("d_paths", k * depth * (a - 1) * E, 16, "out")]


def verify_buffers(depth, a, k):
    return [("d_leaves", k * E, 16, "in"), ("d_indices", k * 8, 8, "in"), ("d_paths", k * depth * (a - 1) * E, 16, "in"), ("d_root", E, 16, "in"),
            ("d_ok", k, 1, "out"), ("d_work", k * (a + 1) * 4 * 8, 16, "scratch")]


def _tree_arena(label, a, n_trees, m, control=False, seed=1):
    """(arena with the leaves in place, leaves, oracle nodes, bytes the call may write)"""
    f, cfg, cr = M.config(label)
    leaves = synth.random_elements(f, n_trees * m, seed=4000 + n_trees + m)
    want = M.forest(cr, leaves, n_trees, a)
    ar = DeviceArena(tree_buffers(want.shape[0]), seed=seed, control=control)
    ar.put("d_nodes", leaves, at=0)
    return ar.upload(), leaves, want, {"d_nodes": (n_trees * m * E, want.shape[0] * E)}       # the leaves rows count as `in`


@pytest.mark.parametrize("label,a,engine", CASES)
def test_merkle_ary_dev(label, a, engine):
    m = a ** 4 if a == 8 else a ** 3
    for control in (False, True):
        for units in (m // a, 1):
            _engine(label, a, engine, units)
        ar, leaves, want, written = _tree_arena(label, a, 1, m, control)
        _lib.check(_lib.lib().pmx_merkle_ary_dev(_ctx(label)._h, ar.ptr("d_nodes"), m, a, _stream()))
        ar.finish(written=written)
        assert np.array_equal(ar.get("d_nodes").reshape(-1, 4), want), (label, control)


@pytest.mark.parametrize("label,a,engine", CASES)
def test_merkle_ary_forest_dev(label, a, engine):
    """65 trees of arity^2 leaves: levels of 65 arity and 65 parents"""
    for control in (False, True):
        for units in (UNITS * a, UNITS):
            _engine(label, a, engine, units)
        ar, leaves, want, written = _tree_arena(label, a, UNITS, a * a, control)
        _lib.check(_lib.lib().pmx_merkle_ary_forest_dev(_ctx(label)._h, ar.ptr("d_nodes"), UNITS, a * a, a, _stream()))
        ar.finish(written=written)
        assert np.array_equal(ar.get("d_nodes").reshape(-1, 4), want), (label, control)


def _path_case(label, a):
    """65 openings over the tree of arity^3 leaves, good and bad ones, with the oracle's verdicts"""
    f, cfg, cr = M.config(label)
    m, depth = a ** 3, 3
    leaves, nodes = M.cached_tree(label, a, m)
    idx = M.path_indices(m, a, UNITS, seed=a)
    paths = M.open_paths(nodes, m, a, idx)
    bad = paths.copy()
    bad[1::2, 1, a - 2, 3] ^= np.uint64(2)                  # every second path: one limb of the last sibling of level 1
    vidx = idx.copy()
    vidx[4::20] += np.uint64(m)                             # an index at or above arity^depth: only the range test fails it
    mine = leaves[idx.astype(np.int64)]
    top = M.climb(cr, mine, vidx, bad, a)
    ok = ((top == nodes[-1]).all(axis=1) & (vidx < np.uint64(m))).astype(np.uint8)
    assert ok[0] == 1 and ok[1] == 0 and ok[4] == 0 and 0 < ok.sum() < UNITS
    return m, depth, nodes, idx, paths, mine, vidx, bad, ok


@pytest.mark.parametrize("label,a,engine", CASES)
def test_merkle_ary_paths_dev(label, a, engine):
    """only d_paths changes; d_indices sits at 8 mod 16"""
    m, depth, nodes, idx, paths, *_ = _path_case(label, a)
    for control in (False, True):
        ar = DeviceArena(paths_buffers(nodes.shape[0], depth, a, UNITS), seed=7, control=control)
        ar.put("d_nodes", nodes)
        ar.put("d_indices", idx)
        ar.upload()
        _lib.check(_lib.lib().pmx_merkle_ary_paths_dev(_ctx(label)._h, ar.ptr("d_nodes"), m, a, ar.ptr("d_indices"), UNITS, ar.ptr("d_paths"),
                                                       _stream()))
        ar.finish()
        assert np.array_equal(ar.get("d_paths").reshape(paths.shape), paths), (label, control)


def _verify_arena(label, a, control=False):
    m, depth, nodes, idx, paths, mine, vidx, bad, ok = _path_case(label, a)
    ar = DeviceArena(verify_buffers(depth, a, UNITS), seed=9, control=control)
    for name, data in (("d_leaves", mine), ("d_indices", vidx), ("d_paths", bad), ("d_root", np.array(nodes[-1]))):
        ar.put(name, data)
    return ar.upload(), depth, ok


def _verify(label, a, ar, depth, shift=None):
    shift = shift or {}
    p = lambda name: ar.ptr(name, shift.get(name, 0))
    return _lib.lib().pmx_merkle_ary_verify_paths_dev(_ctx(label)._h, p("d_leaves"), p("d_indices"), p("d_paths"), depth, a, UNITS, p("d_root"),
                                                      p("d_ok"), p("d_work"), _stream())


@pytest.mark.parametrize("label,a,engine", CASES)
def test_merkle_ary_verify_paths_dev(label, a, engine):
    """d_ok is 65 single bytes at an odd address; d_work is scratch (may be written, not compared)"""
    for control in (False, True):
        _engine(label, a, engine, UNITS)
        ar, depth, ok = _verify_arena(label, a, control)
        if not control:
            assert ar.ptr("d_ok") % 2 == 1
        _lib.check(_verify(label, a, ar, depth))
        ar.finish()
        got = ar.get("d_ok", np.uint8)
        assert np.array_equal(got, ok), (label, control)
        assert (got.min(), got.max()) == (0, 1)


@pytest.mark.parametrize("label,a,engine", CASES)
def test_an_element_pointer_at_8_mod_16_is_refused(label, a, engine):
    L, h, s = _lib.lib(), _ctx(label)._h, _stream()

    def refused(ar, rc, what):
        assert rc == _lib.PMX_ERR_ARG, (what, L.pmx_last_error())
        assert b"16-byte aligned" in L.pmx_last_error(), (what, L.pmx_last_error())
        ar.unchanged()

    ar, leaves, want, written = _tree_arena(label, a, 1, a * a)
    assert ar.ptr("d_nodes", 8) % 16 == 8
    refused(ar, L.pmx_merkle_ary_dev(h, ar.ptr("d_nodes", 8), a * a, a, s), "pmx_merkle_ary_dev")
    refused(ar, L.pmx_merkle_ary_forest_dev(h, ar.ptr("d_nodes", 8), 1, a * a, a, s), "pmx_merkle_ary_forest_dev")

    m, depth, nodes, idx, paths, *_ = _path_case(label, a)
    ar = DeviceArena(paths_buffers(nodes.shape[0], depth, a, UNITS), seed=7)
    ar.put("d_nodes", nodes)
    ar.put("d_indices", idx)
    ar.upload()
    for name in ("d_nodes", "d_paths"):
        ptr = {n: ar.ptr(n, 8 if n == name else 0) for n in ("d_nodes", "d_indices", "d_paths")}
        refused(ar, L.pmx_merkle_ary_paths_dev(h, ptr["d_nodes"], m, a, ptr["d_indices"], UNITS, ptr["d_paths"], s), name)

    ar, depth, ok = _verify_arena(label, a)
    for name in ("d_leaves", "d_paths", "d_work", "d_root"):
        refused(ar, _verify(label, a, ar, depth, shift={name: 8}), name)
    # the call itself still works on these buffers
    _lib.check(_verify(label, a, ar, depth))
    ar.finish()
    assert np.array_equal(ar.get("d_ok", np.uint8), ok)
