"""The host-only pieces of the trees over any number of leaves (include/poseidon_mi355x.h: pmx_merkle_ragged_shape,
pmx_merkle_ragged_paths, every refusal that needs no device) and the data fixture tests/golden/merkle_ragged_vectors.json.  No kernel
runs here; expected values come from the oracles, never from the product: shapes by plain arithmetic, node arrays from the C port level
by level with the short parent as an absorb of the children that exist (tests/merkle_ragged_oracle.py), the fixture from the Python
big-integer oracle (tests/golden/make_merkle_ragged_golden.py).  The index arithmetic of the two bounded gather kernels
(paths_gather_ragged_kernel, node_children_bounded_kernel in sponge_amd/csrc/pmx_tree_moves.hip) is restated here lane by lane."""
import ctypes

import numpy as np
import pytest

import sponge_amd as S
from sponge_amd import _lib
from oracle import cref
from oracle import poseidon_oracle as O

import merkle_ary_oracle as MA
import merkle_ragged_oracle as M
from helpers import FIELDS, golden

SIZE_MAX = (1 << 64) - 1


def _shape(n_leaves, arity):
    depth, nodes = ctypes.c_size_t(12345), ctypes.c_size_t(12345)
    rc = _lib.lib().pmx_merkle_ragged_shape(n_leaves, arity, ctypes.byref(depth), ctypes.byref(nodes))
    return rc, depth.value, nodes.value


def _void(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_shape_against_plain_arithmetic():
    for a in range(2, 17):
        for n in range(1, 301):
            depth, nodes, w = 0, n, n
            while w > 1:
                w = (w + a - 1) // a
                nodes += w
                depth += 1
            assert _shape(n, a) == (_lib.PMX_OK, depth, nodes), (a, n)
            assert M.shape(n, a) == (depth, nodes)
    # the rows people commit to: 2^20 and 2^22 leaves under the octal tree
    assert _shape(1 << 20, 8) == (_lib.PMX_OK, 7, sum([1 << 20, 1 << 17, 1 << 14, 1 << 11, 1 << 8, 32, 4, 1]))
    assert _shape(1 << 22, 8) == (_lib.PMX_OK, 8, sum([1 << 22, 1 << 19, 1 << 16, 1 << 13, 1 << 10, 128, 16, 2, 1]))
    assert sum(M.widths(1 << 20, 8)[1:]) == 149797, "the permutations of the octal tree over 2^20 leaves"


@pytest.mark.parametrize("a,m", [(8, 512), (3, 81), (2, 64), (15, 225), (4, 1)])
def test_shape_of_a_power_of_the_arity_is_the_ary_shape(a, m):
    depth, nodes = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(_lib.lib().pmx_merkle_ary_shape(m, a, ctypes.byref(depth), ctypes.byref(nodes)))
    assert _shape(m, a) == (_lib.PMX_OK, depth.value, nodes.value) and MA.shape(m, a) == M.shape(m, a)


def test_shape_refusals_write_nothing():
    for n, a in ((0, 2), (0, 8), (1, 0), (1, 1), (100, 1), (100, 0), (SIZE_MAX, 8), (1 << 62, 2), (SIZE_MAX // 32, 16), (1 << 59, 8)):
        rc, depth, nodes = _shape(n, a)
        assert rc == _lib.PMX_ERR_ARG, (n, a)
        assert (depth, nodes) == (12345, 12345), "a refused shape writes nothing"
    assert _shape(1 << 59, 8)[0] == _lib.PMX_ERR_ARG and b"overflow" in _lib.lib().pmx_last_error()
    # the largest leaf count whose node array still fits, exactly, at arity 2: n + ceil(n / 2) + ... <= SIZE_MAX / 32
    lo, hi = 1, SIZE_MAX // 32
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if M.shape(mid, 2)[1] <= SIZE_MAX // 32 else (lo, mid - 1)
    assert _shape(lo, 2)[0] == _lib.PMX_OK and _shape(lo + 1, 2)[0] == _lib.PMX_ERR_ARG
    assert _lib.lib().pmx_merkle_ragged_shape(9, 8, None, None) == _lib.PMX_ERR_ARG


# (label, arity, leaves): rate >= arity; the oracle builds the node array, the library only gathers
GATHER = [("t9-bn254", 8, 513), ("t9-bn254", 8, 1024), ("t4", 3, 100), ("t6", 4, 1000), ("lds-t16", 15, 226), ("t3", 2, 100), ("t9-bn254", 8, 9),
          ("t9-bn254", 8, 2), ("t9-bn254", 8, 1)]


@pytest.mark.parametrize("label,a,m", GATHER)
def test_paths_gather_equals_the_oracle_and_the_oracle_climbs_to_the_root(label, a, m):
    f, cfg, cr = M.config(label)
    leaves, nodes = M.cached_tree(label, a, m)
    depth, n_nodes = M.shape(m, a)
    assert nodes.shape == (n_nodes, 4) and np.array_equal(nodes[:m], leaves)
    idx = M.path_indices(m, a, 40, seed=m)
    buf = np.full(max(len(idx) * depth * (a - 1) * 4, 4), 0xDEADBEEF, dtype=np.uint64)      # (never an empty allocation: depth 0)
    paths = buf[:len(idx) * depth * (a - 1) * 4].reshape(len(idx), depth, a - 1, 4)
    _lib.check(_lib.lib().pmx_merkle_ragged_paths(_void(nodes), m, a, _void(idx), len(idx), _void(buf)))
    want = M.open_paths(nodes, m, a, idx)
    assert np.array_equal(paths, want)
    if m > 1 and any(w % a for w in M.widths(m, a)[:-1]):
        assert (want.reshape(len(idx), -1, 4) == 0).all(axis=2).any(), "some sibling of these openings does not exist"
    # the tree's own climb - every parent absorbs the children that exist - reaches the root
    top = M.climb(cr, leaves[idx.astype(np.int64)], idx, paths, a, m)
    assert np.array_equal(top, np.broadcast_to(nodes[-1], top.shape))
    # and so does the verifier's climb, which reads every slot of a row: the absent ones are zeros
    top = MA.climb(cr, leaves[idx.astype(np.int64)], idx, paths, a)
    assert np.array_equal(top, np.broadcast_to(nodes[-1], top.shape)), "a short parent is the parent of its children padded with zeros"


@pytest.mark.parametrize("label,a,m", [("t9-bn254", 8, 512), ("t4", 3, 81), ("t3", 2, 64)])
def test_a_power_of_the_arity_gathers_what_the_ary_entry_gathers(label, a, m):
    leaves, nodes = MA.cached_tree(label, a, m)
    assert np.array_equal(M.tree(M.config(label)[2], leaves, a), nodes), "the two oracles build one tree"
    idx = MA.path_indices(m, a, 33, seed=m)
    depth = MA.shape(m, a)[0]
    old = np.full((len(idx), depth, a - 1, 4), 1, dtype=np.uint64)
    new = np.full((len(idx), depth, a - 1, 4), 2, dtype=np.uint64)
    _lib.check(_lib.lib().pmx_merkle_ary_paths(_void(nodes), m, a, _void(idx), len(idx), _void(old)))
    _lib.check(_lib.lib().pmx_merkle_ragged_paths(_void(nodes), m, a, _void(idx), len(idx), _void(new)))
    assert old.tobytes() == new.tobytes() and np.array_equal(new, MA.open_paths(nodes, m, a, idx))


def test_paths_gather_refuses_a_bad_index_and_a_bad_shape_and_writes_nothing():
    leaves, nodes = M.cached_tree("t4", 3, 100)
    depth = M.shape(100, 3)[0]
    L = _lib.lib()
    for bad in ([100], [5, 99, 100], [1 << 63], [5, (1 << 64) - 1], [242]):     # (242 < 3^5: in the full tree of this depth, not in this one)
        idx = np.array(bad, dtype=np.uint64)
        paths = np.full((len(bad), depth, 2, 4), 7, dtype=np.uint64)
        assert L.pmx_merkle_ragged_paths(_void(nodes), 100, 3, _void(idx), len(bad), _void(paths)) == _lib.PMX_ERR_ARG, bad
        assert b"out of range" in L.pmx_last_error()
        assert (paths == 7).all(), "a refused gather writes nothing"
    idx = np.array([0], dtype=np.uint64)
    paths = np.full((1, depth, 2, 4), 7, dtype=np.uint64)
    for n, a in ((0, 3), (100, 1), (100, 0), (1 << 62, 3)):
        assert L.pmx_merkle_ragged_paths(_void(nodes), n, a, _void(idx), 1, _void(paths)) == _lib.PMX_ERR_ARG, (n, a)
        assert (paths == 7).all()
    assert L.pmx_merkle_ragged_paths(None, 100, 3, _void(idx), 1, _void(paths)) == _lib.PMX_ERR_ARG
    assert L.pmx_merkle_ragged_paths(_void(nodes), 100, 3, None, 1, _void(paths)) == _lib.PMX_ERR_ARG
    assert L.pmx_merkle_ragged_paths(_void(nodes), 100, 3, _void(idx), 1, None) == _lib.PMX_ERR_ARG
    assert L.pmx_merkle_ragged_paths(None, 100, 3, None, 0, None) == _lib.PMX_OK        # nothing asked for


def test_every_refusal_that_needs_no_device_returns_its_code():
    """null pointers, arity < 2, no leaves, overflowing sizes and a depth that is not the tree's are refused before the device is touched
    (the context argument is checked for NULL first, so NULL stands for `no context` and any non-NULL refusal comes from the shape)"""
    L = _lib.lib()
    buf = np.zeros(64, dtype=np.uint64)
    v = _void(buf)
    ARG = _lib.PMX_ERR_ARG
    # no context
    assert L.pmx_merkle_ragged(None, v, 9, 8, v, v) == ARG
    assert L.pmx_merkle_ragged_dev(None, v, 9, 8, None) == ARG
    assert L.pmx_merkle_ragged_paths_dev(None, v, 9, 8, v, 1, v, None) == ARG
    assert L.pmx_merkle_ragged_verify_paths(None, v, v, v, 2, 8, 9, 1, v, v) == ARG
    assert L.pmx_merkle_ragged_verify_paths_dev(None, v, v, v, 2, 8, 9, 1, v, v, v, None) == ARG
    assert L.pmx_merkle_ragged_update_dev(None, v, 9, 8, v, v, 1, v, None) == ARG
    assert b"null pointer" in L.pmx_last_error()


# ---- the index arithmetic of the bounded gather kernels, lane by lane ---------------------------------------------------------------
def _emulate_paths_gather_ragged(nodes, n_leaves, a, depth, indices):
    """paths_gather_ragged_kernel: one 16-byte quarter per lane (two quarters per element)"""
    k = len(indices)
    flat = np.ascontiguousarray(nodes).reshape(-1, 2)             # uint4 units as pairs of u64
    per_level, out = 2 * (a - 1), np.full((k * depth * 2 * (a - 1), 2), 0x77, dtype=np.uint64)
    per = depth * per_level
    for gid in range(out.shape[0]):
        i = gid // per
        rest = gid - i * per
        level = rest // per_level
        quarter = rest - level * per_level
        sibling, half = quarter >> 1, quarter & 1
        idx, first, width = int(indices[i]), 0, n_leaves
        v = (0, 0)
        if idx < n_leaves:
            for _ in range(level):
                first += width
                width = width // a + (1 if width % a else 0)
                idx //= a
            digit = idx % a
            child = (idx - digit) + (sibling if sibling < digit else sibling + 1)
            if child < width:
                assert first + child < first + width <= nodes.shape[0], "nothing at or beyond the level's end is read"
                v = flat[(first + child) * 2 + half]
        out[gid] = v
    return out.reshape(k, depth, a - 1, 4)


def _emulate_node_children_bounded(nodes, indices, pow_, n_leaves, first, width, a):
    """node_children_bounded_kernel: 2 a lanes per update"""
    k = len(indices)
    flat = np.ascontiguousarray(nodes).reshape(-1, 2)
    out = np.full((k * 2 * a, 2), 0x77, dtype=np.uint64)
    for gid in range(out.shape[0]):
        i = gid // (2 * a)
        quarter = gid - i * 2 * a
        idx = int(indices[i])
        p = idx // pow_ if idx < n_leaves else 0
        child = p * a + (quarter >> 1)
        out[gid] = flat[(first + child) * 2 + (quarter & 1)] if child < width else (0, 0)
        assert child >= width or first + child < first + width
    return out.reshape(k, a, 4)


@pytest.mark.parametrize("label,a,m", [("t3", 2, 100), ("t4", 3, 100), ("t9-bn254", 8, 513), ("lds-t16", 15, 226)])
def test_the_bounded_gather_kernels_index_arithmetic(label, a, m):
    leaves, nodes = M.cached_tree(label, a, m)
    w = M.widths(m, a)
    depth = len(w) - 1
    idx = M.path_indices(m, a, 24, seed=3)
    assert np.array_equal(_emulate_paths_gather_ragged(nodes, m, a, depth, idx), M.open_paths(nodes, m, a, idx))
    wild = np.array([m, (1 << 64) - 1, a ** depth - 1 if a ** depth - 1 >= m else m + 1], dtype=np.uint64)
    assert not _emulate_paths_gather_ragged(nodes, m, a, depth, wild).any(), "an index that names no leaf gets an all-zero path"
    # the update's gather at every level: parent p's row is its children, zeros behind the level's end; an index >= n gathers parent 0's
    upd = np.concatenate([idx, wild])
    first = 0
    for level in range(depth):
        rows = _emulate_node_children_bounded(nodes, upd, a ** (level + 1), m, first, w[level], a)
        for i, index in enumerate(int(x) for x in upd):
            p = index // a ** (level + 1) if index < m else 0
            want = np.zeros((a, 4), dtype=np.uint64)
            have = min(a, w[level] - p * a)
            want[:have] = nodes[first + p * a:first + p * a + have]
            assert np.array_equal(rows[i], want), (level, index)
            assert p < w[level + 1], "floor division nests: index / a^(l+1) is the ancestor's index in its level"
        first += w[level]


def test_the_fixture_equals_the_c_port():
    """tests/golden/merkle_ragged_vectors.json comes from the Python big-integer oracle; the C port must build the same two trees"""
    vectors = golden("merkle_ragged_vectors.json")
    assert sorted(vectors) == ["bls_t5_a5_8_56/arity4/leaves6", "bn254_t9_a5_8_57/arity8/leaves9"]
    for name, v in vectors.items():
        p, bits = FIELDS[v["field"]]
        assert bits == v["prime_bits"]
        a, m = v["arity"], v["n_leaves"]
        assert (name, a, m, v["rate"]) in (("bn254_t9_a5_8_57/arity8/leaves9", 8, 9, 8), ("bls_t5_a5_8_56/arity4/leaves6", 4, 6, 4))
        cr = cref.CRef(O.make_config(p, bits, v["rate"], v["alpha"], v["full_rounds"], v["partial_rounds"]))
        want = cref.elems_to_limbs([int(x, 16) for x in v["nodes"]], p)
        assert want.shape == (M.shape(m, a)[1], 4) and M.widths(m, a) == [m, 2, 1]
        assert np.array_equal(M.tree(cr, want[:m], a), want), name
        # the short parent is the parent of its children padded with zero elements - and so the root does not bind the leaf count
        padded = np.zeros((2 * a, 4), dtype=np.uint64)
        padded[:m] = want[:m]
        assert np.array_equal(cr.hash_batch(padded.reshape(2, a, 4), a, 1, threads=1).reshape(2, 4), want[m:m + 2]), name


def test_python_mirror_shapes_and_offsets():
    """sponge_amd.merkle without a device: the shape of a tree over any number of leaves, a single leaf at any arity"""
    from sponge_amd.poseidon import merkle_ragged_shape
    assert merkle_ragged_shape(1000, 8) == (4, 1000 + 125 + 16 + 2 + 1)
    assert merkle_ragged_shape(512, 8) == (3, 585)
    with pytest.raises(_lib.PmxError):
        merkle_ragged_shape(0, 8)
    f, cfg, cr = M.config("t9-bn254")
    leaf = M.cached_tree("t9-bn254", 8, 1)[0]
    t = S.MerkleTree(cfg, leaf, arity=8)
    assert (t.depth, t.n_leaves, t.ragged, t.level_widths()) == (0, 1, False, [1]) and np.array_equal(t.root, leaf[0])
