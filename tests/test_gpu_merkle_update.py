"""Leaf updates of a resident Merkle tree through the C ABI (pmx_merkle_ary_update_dev, pmx_merkle_ary_update) and MerkleTree.update, on
every engine that serves the trees.  Expected values never come from the product: they are merkle_ary_oracle.tree over the leaf row
with the updates applied - a full rebuild by the C port.

Trees: the shapes of tests/test_gpu_merkle_ary.py (partial waves, one full wave, more than one workgroup, arity below the rate, the
generic S-box, the run-time-width engine, one leaf) and the 2-to-1 tree over 2^17 leaves, where k = 40000 updates are more than the 32768
units the quad engine takes: the gathered rows then go to the window engine of t = 3.
k: 0 and 1; 63, 64, 65 (the wave edge); W - 1, W, W + 1 for the number W of first-level parents (both sides of the switch from gathered
rows to whole levels); every leaf."""
import ctypes

import numpy as np
import pytest
import torch

import sponge_amd as S
from sponge_amd import _lib, synth

import merkle_ary_oracle as M

pytestmark = pytest.mark.gpu

# (label, arity, leaves)
TREES = [
    ("t3", 2, 64),
    ("t3", 2, 1 << 17),
    ("t4", 3, 81),
    ("t6", 4, 1024),
    ("t9-bn254", 8, 512),
    ("t9-bn254", 8, 4096),
    ("t9-bn254", 5, 125),
    ("t9-alpha17", 8, 512),
    ("lds-t16", 15, 225),
    ("t4", 3, 1),
]
SMALL = [t for t in TREES if t[2] <= 4096]
U64 = (1 << 64) - 1
POISON = 0xA5C3A5C3A5C3A5C3


def _counts(a, m):
    W = m // a
    ks = {0, 1, 63, 64, 65, W - 1, W, W + 1, m}
    if m == 1 << 17:
        ks.add(40000)
    return sorted(k for k in ks if 0 <= k <= m)


CASES = [(label, a, m, k) for label, a, m in TREES for k in _counts(a, m)]


def _ctx(label):
    return M.config(label)[1].context()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    """a host array on the device, as bytes"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def _host(t, dtype=np.uint64):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype)


def _indices(m, k, seed):
    """k distinct leaves, 0 and m - 1 among them from k = 2 on"""
    rng = np.random.default_rng(seed)
    idx = rng.choice(m, k, replace=False).astype(np.uint64)
    if k >= 2:
        rest = [int(x) for x in idx if int(x) not in (0, m - 1)]
        idx = np.array([m - 1, 0] + rest[:k - 2], dtype=np.uint64)
        rng.shuffle(idx)
    return idx


def _applied(leaves, idx, new):
    out = np.array(leaves, dtype=np.uint64)
    for i, j in enumerate(int(x) for x in idx):      # in call order: the last one wins
        out[j] = new[i]
    return out


def _update_dev(label, a, m, image, idx, new):
    """pmx_merkle_ary_update_dev on a copy of `image`; the node array afterwards"""
    k = len(idx)
    d_nodes, d_idx, d_new = _dev(image), _dev(idx if k else np.zeros(1, np.uint64)), _dev(new if k else np.zeros(4, np.uint64))
    d_work = torch.full((max(k, 1) * (a + 1) * 4,), 0x77, dtype=torch.int64, device="cuda:0")
    _ctx(label).merkle_ary_update_dev(d_nodes.data_ptr(), m, a, d_idx.data_ptr(), d_new.data_ptr(), k, d_work.data_ptr(), _stream())
    return _host(d_nodes).reshape(-1, 4)


@pytest.mark.parametrize("label,a,m,k", CASES)
def test_updated_tree_equals_the_rebuild(label, a, m, k):
    f, cfg, cr = M.config(label)
    leaves, old = M.cached_tree(label, a, m)
    idx = _indices(m, k, seed=m + 31 * k)
    new = synth.random_elements(f, max(k, 1), seed=900 + m + k)[:k]
    want = M.tree(cr, _applied(leaves, idx, new), a)
    assert k == 0 or not np.array_equal(want[-1], old[-1])
    got = _update_dev(label, a, m, old, idx, new)
    assert np.array_equal(got, want), ("pmx_merkle_ary_update_dev", label, a, m, k)
    nodes = old.copy()
    root = _ctx(label).merkle_ary_update(nodes, m, a, idx, new)
    assert np.array_equal(nodes, want), ("pmx_merkle_ary_update", label, a, m, k)
    assert np.array_equal(root, want[-1])


def test_gathered_rows_beyond_the_quad_range_take_the_window_engine():
    """what the 2^17-leaf case with k = 40000 rests on: 40000 units of the 2-to-1 compression are no longer the quad engine's"""
    info = _lib.PmxEngineInfo()
    for n, want in ((32768, b"QuadEngine"), (40000, b"HybridEngine<3,5")):
        _lib.check(_lib.lib().pmx_ctx_engine_info(_ctx("t3")._h, _lib.OP_COMPRESS, n, 2, ctypes.byref(info)))
        assert info.engine.startswith(want), (n, info.engine)
    assert 40000 < (1 << 17) // 2


def _ancestors(idx, a, m):
    """node-array rows of the leaves idx and of everything above them"""
    depth, _ = M.shape(m, a)
    rows, first, width = set(), 0, m
    for level in range(depth + 1):
        rows |= {first + int(j) // a ** level for j in idx}
        first, width = first + width, width // a
    return rows


@pytest.mark.parametrize("label,a,m", TREES)
def test_nodes_that_are_no_ancestor_are_not_written(label, a, m):
    """every node that is neither an updated leaf nor above one holds a poison pattern before the call and must hold it afterwards.
    k is below every switch to whole levels that could reach such a node: one update (the only whole level is the root's), and one
    update in each of the arity subtrees under the root (the whole levels are the root's and its children's, all of them ancestors)."""
    f, cfg, cr = M.config(label)
    leaves, old = M.cached_tree(label, a, m)
    depth, n_nodes = M.shape(m, a)
    rng = np.random.default_rng(m)
    sets = [[int(rng.integers(0, m))]]
    if depth >= 2:
        sub = m // a
        sets.append([c * sub + int(rng.integers(0, sub)) for c in range(a)])
    for raw in sets:
        idx = np.array(raw, dtype=np.uint64)
        new = synth.random_elements(f, len(idx), seed=m + len(idx))
        keep = np.array(sorted(set(range(n_nodes)) - _ancestors(idx, a, m)), dtype=np.int64)
        image = old.copy()
        image[keep] = np.uint64(POISON)
        got = _update_dev(label, a, m, image, idx, new)
        assert (got[keep] == np.uint64(POISON)).all(), (label, a, m, len(idx))
        assert np.array_equal(got[idx.astype(np.int64)], new)
        assert not (got[sorted(_ancestors(idx, a, m))] == np.uint64(POISON)).any()


@pytest.mark.parametrize("label,a,m", SMALL)
def test_device_entry_edge_cases(label, a, m):
    """equal-index equal-leaf duplicates, many updates under one parent, and indices that name no leaf (n_leaves, 2^64 - 1: ignored)"""
    f, cfg, cr = M.config(label)
    leaves, old = M.cached_tree(label, a, m)
    fresh = synth.random_elements(f, 2 * a + 8, seed=77 + m)
    parent = (m // a) // 2                                     # all children of one parent, the first of them twice
    under = [min(parent * a + c, m - 1) for c in range(a)]
    real = list(dict.fromkeys(under + [0, m - 1]))
    value = {j: fresh[n] for n, j in enumerate(real)}
    order = real + [under[0], m, real[-1], U64, m, under[0]]
    idx = np.array(order, dtype=np.uint64)
    new = np.stack([value[j] if j < m else fresh[-1 - (n % 3)] for n, j in enumerate(order)])
    want = M.tree(cr, _applied(leaves, np.array(real, dtype=np.uint64), np.stack([value[j] for j in real])), a)
    got = _update_dev(label, a, m, old, idx, new)
    assert np.array_equal(got, want), (label, a, m)
    # indices that name no leaf alone: the tree stays as it was
    only_bad = np.array([m, U64, m + 1], dtype=np.uint64)
    assert np.array_equal(_update_dev(label, a, m, old, only_bad, fresh[:3]), old)


@pytest.mark.parametrize("label,a,m", SMALL)
def test_host_entry_duplicates_are_sequential_updates(label, a, m):
    f, cfg, cr = M.config(label)
    leaves, old = M.cached_tree(label, a, m)
    rng = np.random.default_rng(5 * m)
    idx = np.concatenate([rng.integers(0, m, 70), [0, m - 1, 0, m - 1, m // 2, 0]]).astype(np.uint64)
    new = synth.random_elements(f, len(idx), seed=55 + m)
    assert len(set(int(x) for x in idx)) < len(idx)
    want = M.tree(cr, _applied(leaves, idx, new), a)
    nodes = old.copy()
    root = _ctx(label).merkle_ary_update(nodes, m, a, idx, new)
    assert np.array_equal(nodes, want) and np.array_equal(root, want[-1])
    # an index that names no leaf: refused by name, nothing changes
    bad = idx.copy()
    bad[-2] = m
    with pytest.raises(_lib.PmxError, match="out of range"):
        _ctx(label).merkle_ary_update(nodes, m, a, bad, new)
    assert np.array_equal(nodes, want)
    # root may be NULL
    again = old.copy()
    _lib.check(_lib.lib().pmx_merkle_ary_update(_ctx(label)._h, ctypes.c_void_p(again.ctypes.data), m, a, ctypes.c_void_p(idx.ctypes.data),
                                                ctypes.c_void_p(new.ctypes.data), len(idx), None))
    assert np.array_equal(again, want)


@pytest.mark.parametrize("m,k", [(64, 1), (64, 33), (4096, 65), (4096, 2048)])
def test_arity_two_is_the_2to1_tree_over_the_new_leaves(m, k):
    f, cfg, cr = M.config("t3")
    leaves, old = M.cached_tree("t3", 2, m)
    idx = _indices(m, k, seed=k)
    new = synth.random_elements(f, k, seed=m + k)
    after = _applied(leaves, idx, new)
    rebuilt, root = _ctx("t3").merkle_2to1(after)
    assert np.array_equal(rebuilt, cr.merkle(after, threads=0))
    assert _update_dev("t3", 2, m, old, idx, new).tobytes() == rebuilt.tobytes()
    nodes = old.copy()
    assert _ctx("t3").merkle_ary_update(nodes, m, 2, idx, new).tobytes() == root.tobytes() and nodes.tobytes() == rebuilt.tobytes()


@pytest.mark.parametrize("label,a,m", [("t3", 2, 64), ("t4", 3, 81), ("t9-bn254", 8, 512), ("t9-bn254", 5, 125), ("lds-t16", 15, 225), ("t4", 3, 1)])
def test_tree_update_then_openings_verify_against_the_new_root(label, a, m):
    f, cfg, cr = M.config(label)
    leaves, old = M.cached_tree(label, a, m)
    tree = S.MerkleTree(cfg, leaves, arity=a)
    assert np.array_equal(tree.nodes, old)
    k = min(m, 9)
    idx = _indices(m, k, seed=a)
    new = synth.random_elements(f, k, seed=3 * m)
    tree.update(idx, new)
    want = M.tree(cr, _applied(leaves, idx, new), a)
    assert np.array_equal(tree.nodes, want) and np.array_equal(tree.root, want[-1])
    paths = tree.paths(idx)
    assert S.merkle.verify_paths(cfg, new, idx, paths, tree.root, arity=a).all()
    assert not S.merkle.verify_paths(cfg, leaves[idx.astype(np.int64)], idx, paths, tree.root, arity=a).any()
    assert not S.merkle.verify_paths(cfg, new, idx, paths, old[-1], arity=a).any()
