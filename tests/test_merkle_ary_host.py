"""The host-only pieces of the arity-k Merkle entry points (include/poseidon_mi355x.h: pmx_merkle_ary_shape, pmx_merkle_ary_paths) and
the data fixture tests/golden/merkle_ary_vectors.json.  No kernel runs here; expected values come from the oracles, never from the
product: shapes by plain arithmetic, node arrays from the C port's batch hash level by level (tests/merkle_ary_oracle.py), the fixture
from the Python big-integer oracle (tests/golden/make_merkle_ary_golden.py)."""
import ctypes

import numpy as np
import pytest

from sponge_amd import _lib
from oracle import cref
from oracle import poseidon_oracle as O

import merkle_ary_oracle as M
from helpers import FIELDS, golden

ARITIES = [2, 3, 8, 15]
SIZE_MAX = (1 << 64) - 1


def _shape(n_leaves, arity):
    depth, nodes = ctypes.c_size_t(12345), ctypes.c_size_t(12345)
    rc = _lib.lib().pmx_merkle_ary_shape(n_leaves, arity, ctypes.byref(depth), ctypes.byref(nodes))
    return rc, depth.value, nodes.value


def _void(a):
    return ctypes.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("a", ARITIES)
def test_shape_of_every_power_of_the_arity(a):
    assert _shape(1, a) == (_lib.PMX_OK, 0, 1)                  # one leaf is its own root
    n, depth = 1, 0
    while n * a * 32 * 2 <= SIZE_MAX:                           # (a node array is below 2 n elements of 32 bytes)
        n, depth = n * a, depth + 1
        want_nodes = (a ** (depth + 1) - 1) // (a - 1)
        assert _shape(n, a) == (_lib.PMX_OK, depth, want_nodes), (a, depth)
        assert M.shape(n, a) == (depth, want_nodes)
    assert depth >= 14


@pytest.mark.parametrize("a", ARITIES)
def test_shape_refuses_what_is_no_power_of_the_arity(a):
    candidates = [0, a + 1, a * a - 1, a * a + a, 2 * a ** 3, a ** 5 + 1, 48, 2 * a, a ** 4 - a, 3 * a ** 7, (1 << 64) - 1, 1 << 62, 3 ** 39 * 2]
    bad = [n for n in candidates if M_log(n, a) < 0]
    assert len(bad) >= 9
    for n in bad:
        rc, depth, nodes = _shape(n, a)
        assert rc == _lib.PMX_ERR_ARG, (a, n)
        assert (depth, nodes) == (12345, 12345), "a refused shape writes nothing"
    for arity in (0, 1):
        assert _shape(1, arity)[0] == _lib.PMX_ERR_ARG
        assert _shape(4, arity)[0] == _lib.PMX_ERR_ARG


def M_log(n, a):
    """the exponent if n is a power of a, else -1"""
    d = 0
    while n > 1 and n % a == 0:
        n, d = n // a, d + 1
    return d if n == 1 else -1


@pytest.mark.parametrize("a", ARITIES)
def test_shape_refuses_a_node_array_whose_bytes_overflow(a):
    """the largest power of the arity in a size_t: its node count still fits 64 bits, its byte size does not"""
    n = 1
    while n * a <= SIZE_MAX:
        n *= a
    assert (a ** (M_log(n, a) + 1) - 1) // (a - 1) * 32 > SIZE_MAX
    rc, depth, nodes = _shape(n, a)
    assert rc == _lib.PMX_ERR_ARG and (depth, nodes) == (12345, 12345)
    assert b"overflow" in _lib.lib().pmx_last_error()
    # and the first power whose bytes overflow, exactly
    n = 1
    while (a ** (M_log(n, a) + 1) - 1) // (a - 1) * 32 <= SIZE_MAX:
        ok_n, n = n, n * a
    assert _shape(ok_n, a)[0] == _lib.PMX_OK and _shape(n, a)[0] == _lib.PMX_ERR_ARG
    assert _lib.lib().pmx_merkle_ary_shape(8, 2, None, None) == _lib.PMX_ERR_ARG


# (label, arity, leaves): rate >= arity; the oracle builds the node array, the library only gathers
GATHER = [("t4", 3, 81), ("t9-bn254", 8, 512), ("t9-bn254", 5, 125), ("lds-t16", 15, 225), ("t3", 2, 64), ("t9-bn254", 8, 1)]


@pytest.mark.parametrize("label,a,m", GATHER)
def test_paths_gather_puts_every_sibling_where_the_index_arithmetic_says(label, a, m):
    f, cfg, cr = M.config(label)
    leaves, nodes = M.cached_tree(label, a, m)
    depth, n_nodes = M.shape(m, a)
    assert nodes.shape == (n_nodes, 4) and np.array_equal(nodes[:m], leaves)
    idx = M.path_indices(m, a, 40, seed=m)
    assert {0, m - 1} <= set(int(i) for i in idx) and (m == 1 or {int(i) % a for i in idx} == set(range(a)))
    buf = np.full(max(len(idx) * depth * (a - 1) * 4, 4), 0xDEADBEEF, dtype=np.uint64)      # (never an empty allocation: depth 0)
    paths = buf[:len(idx) * depth * (a - 1) * 4].reshape(len(idx), depth, a - 1, 4)
    _lib.check(_lib.lib().pmx_merkle_ary_paths(_void(nodes), m, a, _void(idx), len(idx), _void(buf)))
    assert np.array_equal(paths, M.open_paths(nodes, m, a, idx))
    # re-hashing every leaf up its path with the oracle reaches the root
    top = M.climb(cr, leaves[idx.astype(np.int64)], idx, paths, a)
    assert np.array_equal(top, np.broadcast_to(nodes[-1], top.shape))


def test_paths_gather_refuses_a_bad_index_and_a_bad_shape_and_writes_nothing():
    leaves, nodes = M.cached_tree("t4", 3, 81)
    L = _lib.lib()
    for bad in ([81], [5, 80, 81], [1 << 63], [5, (1 << 64) - 1]):
        idx = np.array(bad, dtype=np.uint64)
        paths = np.full((len(bad), 4, 2, 4), 7, dtype=np.uint64)
        assert L.pmx_merkle_ary_paths(_void(nodes), 81, 3, _void(idx), len(bad), _void(paths)) == _lib.PMX_ERR_ARG, bad
        assert b"out of range" in L.pmx_last_error()
        assert (paths == 7).all(), "a refused gather writes nothing"
    idx = np.array([0], dtype=np.uint64)
    paths = np.full((1, 4, 2, 4), 7, dtype=np.uint64)
    for n, a in ((80, 3), (0, 3), (54, 3), (81, 1), (81, 0), (81, 2), (81, 27 * 27)):
        assert L.pmx_merkle_ary_paths(_void(nodes), n, a, _void(idx), 1, _void(paths)) == _lib.PMX_ERR_ARG, (n, a)
        assert (paths == 7).all()
    assert L.pmx_merkle_ary_paths(None, 81, 3, _void(idx), 1, _void(paths)) == _lib.PMX_ERR_ARG
    assert L.pmx_merkle_ary_paths(_void(nodes), 81, 3, None, 1, _void(paths)) == _lib.PMX_ERR_ARG
    assert L.pmx_merkle_ary_paths(_void(nodes), 81, 3, _void(idx), 1, None) == _lib.PMX_ERR_ARG
    assert L.pmx_merkle_ary_paths(None, 81, 3, None, 0, None) == _lib.PMX_OK        # nothing asked for


@pytest.mark.parametrize("m", [1, 2, 64, 1024])
def test_arity_two_is_the_2to1_gather_byte_for_byte(m):
    f, cfg, cr = M.config("t3")
    leaves, nodes = M.cached_tree("t3", 2, m)
    assert m == 1 or np.array_equal(nodes, cr.merkle(leaves, threads=0)), "the level-by-level oracle is the C port's own 2-to-1 tree"
    depth = m.bit_length() - 1
    idx = M.path_indices(m, 2, 33, seed=m)
    old = np.full((len(idx), depth, 4), 1, dtype=np.uint64)
    new = np.full((len(idx), depth, 1, 4), 2, dtype=np.uint64)
    L = _lib.lib()
    _lib.check(L.pmx_merkle_paths(_void(nodes), m, _void(idx), len(idx), _void(old)))
    _lib.check(L.pmx_merkle_ary_paths(_void(nodes), m, 2, _void(idx), len(idx), _void(new)))
    assert old.tobytes() == new.tobytes()


def test_the_fixture_equals_the_c_port():
    """tests/golden/merkle_ary_vectors.json comes from the Python big-integer oracle; the C port must build the same two trees"""
    vectors = golden("merkle_ary_vectors.json")
    assert sorted(vectors) == ["bls_t5_a5_8_56/arity4", "bn254_t9_a5_8_57/arity8"]
    for name, v in vectors.items():
        p, bits = FIELDS[v["field"]]
        assert bits == v["prime_bits"]
        a, m = v["arity"], v["n_leaves"]
        assert (name, a, m, v["rate"]) in (("bn254_t9_a5_8_57/arity8", 8, 64, 8), ("bls_t5_a5_8_56/arity4", 4, 16, 4))
        cr = cref.CRef(O.make_config(p, bits, v["rate"], v["alpha"], v["full_rounds"], v["partial_rounds"]))
        want = cref.elems_to_limbs([int(x, 16) for x in v["nodes"]], p)
        assert want.shape == (M.shape(m, a)[1], 4)
        assert np.array_equal(M.tree(cr, want[:m], a), want), name


def test_python_mirror_shapes_and_offsets():
    """sponge_amd.merkle without a device: a single leaf is its own tree at any arity; level_offset is the header's row formula"""
    import sponge_amd as S
    f, cfg, cr = M.config("t9-bn254")
    leaf = M.cached_tree("t9-bn254", 8, 1)[0]
    for a in (2, 8):
        t = S.MerkleTree(cfg, leaf, arity=a)
        assert (t.depth, t.n_leaves, t.arity) == (0, 1, a) and np.array_equal(t.root, leaf[0]) and np.array_equal(t.nodes, leaf)
        assert t.paths([0]).shape == ((1, 0, 4) if a == 2 else (1, 0, a - 1, 4))
    assert S.MerkleTree(cfg, leaf).arity == 2
    from sponge_amd.poseidon import merkle_ary_shape
    assert merkle_ary_shape(512, 8) == (3, 585)
    with pytest.raises(_lib.PmxError):
        merkle_ary_shape(500, 8)
