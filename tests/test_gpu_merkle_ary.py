"""Merkle trees, forests, openings and path verification of any arity through the C ABI (pmx_merkle_ary*), on every engine that serves
them.  Expected values never come from the product: node arrays are the C port's batch hash applied level by level
(tests/merkle_ary_oracle.py), and tests/golden/merkle_ary_vectors.json pins two trees from the Python big-integer oracle.

Shapes are the smallest that reach each way the kernel can go wrong: partial waves (81 leaves at arity 3: levels of 27, 9, 3, 1
parents), one full workgroup down to one lane (1024 leaves at arity 4: 256 / 64 / 16 / 4 / 1), exactly one full wave (512 leaves at
arity 8: 64, 8, 1), more than one workgroup (4096 at arity 8: 512 parents), arity = rate, arity below the rate (the lanes behind the last
child must stay zero), the generic S-box, the run-time-width engine at t = 16, and arity 2 through the new entries on both sides of the
quad engine's range."""
import ctypes

import numpy as np
import pytest
import torch

import sponge_amd as S
from sponge_amd import _lib, synth
from oracle import cref
from oracle import poseidon_oracle as O

import merkle_ary_oracle as M
from helpers import FIELDS, golden

pytestmark = pytest.mark.gpu

# (label, arity, leaves)
TREES = [
    ("t4", 3, 81),
    ("t6", 4, 1024),
    ("t6", 5, 125),
    ("t9-bn254", 8, 512),
    ("t9-bn254", 8, 4096),
    ("t9-bn254", 5, 125),
    ("t9-bn254", 3, 81),
    ("t9-alpha17", 8, 512),
    ("lds-t16", 15, 225),
    ("lds-t16", 7, 343),
    ("t3", 2, 64),
    ("t3", 2, 4096),
]
FORESTS = [("t9-bn254", 3, 5, 27), ("t9-bn254", 8, 3, 64)]      # (label, arity, trees, leaves per tree)
ENGINE = {"t4": b"HybridEngine<4,5", "t6": b"HybridEngine<6,5", "t9-bn254": b"HybridEngine<9,5", "t9-alpha17": b"HybridEngine<9,0",
          "lds-t16": b"LdsEngine<5>", "t3": b"QuadEngine<5>"}
PATH_TREES = [("t4", 3, 81), ("t9-bn254", 8, 512), ("t9-bn254", 5, 125), ("lds-t16", 15, 225), ("t3", 2, 64)]
PATH_COUNTS = [1, 65, 257]


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


def _engine(label, n, length):
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(_ctx(label)._h, _lib.OP_COMPRESS, n, length, ctypes.byref(info)))
    return info


# ---- every node -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,a,m", TREES)
def test_every_node_of_the_tree_equals_the_oracle(label, a, m):
    f, cfg, cr = M.config(label)
    leaves, want = M.cached_tree(label, a, m)
    nodes, root = _ctx(label).merkle_ary(leaves, a)
    assert np.array_equal(nodes, want), (label, a, m)
    assert np.array_equal(root, want[-1])
    _, only_root = _ctx(label).merkle_ary(leaves, a, want_nodes=False)
    assert np.array_equal(only_root, want[-1])
    if a == 2:      # the new entries at arity 2 ARE the 2-to-1 tree: same bytes as pmx_merkle_2to1 and as the C port's own tree
        old_nodes, old_root = _ctx(label).merkle_2to1(leaves)
        assert nodes.tobytes() == old_nodes.tobytes() and root.tobytes() == old_root.tobytes()
        assert np.array_equal(nodes, cr.merkle(leaves, threads=0))


@pytest.mark.parametrize("label,a,m", TREES)
def test_the_device_entry_equals_the_host_entry(label, a, m):
    leaves, want = M.cached_tree(label, a, m)
    depth, n_nodes = M.shape(m, a)
    image = np.full((n_nodes, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    image[:m] = leaves
    d = _dev(image)
    _ctx(label).merkle_ary_dev(d.data_ptr(), m, a, _stream())
    assert np.array_equal(_host(d).reshape(n_nodes, 4), want), (label, a, m)


@pytest.mark.parametrize("label,a,m", TREES)
def test_the_engine_report_names_the_engine_of_the_level(label, a, m):
    """pmx_ctx_engine_info(PMX_OP_COMPRESS, n, arity) names the family select_engine gives for (PMX_OP_COMPRESS, n): the arity does
    not enter the choice"""
    n = m // a
    while n >= 1:
        with_arity, plain = _engine(label, n, a), _engine(label, n, 0)
        assert with_arity.engine == plain.engine and with_arity.engine.startswith(ENGINE[label]), (label, n, with_arity.engine)
        assert (with_arity.threads, with_arity.waves_per_simd, with_arity.lds_bytes, with_arity.launches) == \
               (plain.threads, plain.waves_per_simd, plain.lds_bytes, plain.launches)
        n //= a


def test_arity_two_above_the_quad_range_takes_the_window_engine():
    """t = 3: levels of more than 32768 compressions leave the quad engine - the 2-to-1 launch, whatever entry asked for it"""
    assert _engine("t3", 32768, 2).engine.startswith(b"QuadEngine") and _engine("t3", 32769, 2).engine.startswith(b"HybridEngine<3,5")
    leaves, want = M.cached_tree("t3", 2, 1 << 17)         # level 1: 65536 compressions
    nodes, root = _ctx("t3").merkle_ary(leaves, 2)
    assert np.array_equal(nodes, want)


@pytest.mark.parametrize("label,a,n_trees,m", FORESTS)
def test_every_node_of_the_forest_equals_the_oracle(label, a, n_trees, m):
    f, cfg, cr = M.config(label)
    leaves = synth.random_elements(f, n_trees * m, seed=0xF0 + n_trees)
    want = M.forest(cr, leaves, n_trees, a)
    depth, tree_nodes = M.shape(m, a)
    assert want.shape[0] == n_trees * tree_nodes
    # the header's row formula, tree by tree against the single-tree oracle
    for b in range(n_trees):
        single = M.tree(cr, leaves[b * m:(b + 1) * m], a)
        first = 0
        for level in range(depth + 1):
            w = m // a ** level
            row = n_trees * sum(m // a ** l for l in range(level)) + b * w
            assert np.array_equal(want[row:row + w], single[first:first + w])
            first += w
    nodes, roots = _ctx(label).merkle_ary_forest(leaves, n_trees, a)
    assert np.array_equal(nodes, want) and np.array_equal(roots, want[-n_trees:])
    image = np.full_like(want, 0x33)
    image[:n_trees * m] = leaves
    d = _dev(image)
    _ctx(label).merkle_ary_forest_dev(d.data_ptr(), n_trees, m, a, _stream())
    assert np.array_equal(_host(d).reshape(-1, 4), want)


@pytest.mark.parametrize("label,a", [("t4", 3), ("t9-bn254", 8), ("lds-t16", 15), ("t3", 2)])
def test_a_single_leaf_is_its_own_tree(label, a):
    leaf, _ = M.cached_tree(label, a, 1)
    nodes, root = _ctx(label).merkle_ary(leaf, a)
    assert np.array_equal(nodes, leaf) and np.array_equal(root, leaf[0])
    nodes, roots = _ctx(label).merkle_ary_forest(np.concatenate([leaf, leaf, leaf]), 3, a)
    assert np.array_equal(nodes, np.concatenate([leaf, leaf, leaf])) and np.array_equal(roots, nodes)
    d = _dev(leaf)
    _ctx(label).merkle_ary_dev(d.data_ptr(), 1, a, _stream())
    assert np.array_equal(_host(d).reshape(1, 4), leaf)


def test_the_fixture_of_the_big_integer_oracle():
    """tests/golden/merkle_ary_vectors.json: the octal tree of the t = 9 config and the quaternary one of the rate-4 default"""
    for name, v in golden("merkle_ary_vectors.json").items():
        p, bits = FIELDS[v["field"]]
        f = S.BN254_FR if v["field"] == "bn254_fr" else S.BLS12_381_FR
        cfg = S.poseidon_config_from_lfsr(f, v["rate"], v["alpha"], v["full_rounds"], v["partial_rounds"])
        want = cref.elems_to_limbs([int(x, 16) for x in v["nodes"]], p)
        nodes, root = cfg.context().merkle_ary(want[:v["n_leaves"]], v["arity"])
        assert np.array_equal(nodes, want), name
        tree = S.MerkleTree(cfg, want[:v["n_leaves"]], arity=v["arity"])
        assert np.array_equal(tree.nodes, want) and np.array_equal(tree.root, want[-1])
        assert tree.level_offset(1) == v["n_leaves"] and tree.level_offset(tree.depth) == want.shape[0] - 1


# ---- openings -----------------------------------------------------------------------------------------------------------------
def _gather_dev(label, a, m, nodes, idx):
    depth, _ = M.shape(m, a)
    k = len(idx)
    d_nodes, d_idx = _dev(nodes), _dev(idx)
    d_paths = _dev(np.full(max(k * depth * (a - 1) * 4, 4), 0x77, dtype=np.uint64))
    _ctx(label).merkle_ary_paths_dev(d_nodes.data_ptr(), m, a, d_idx.data_ptr(), k, d_paths.data_ptr(), _stream())
    return _host(d_paths)[:k * depth * (a - 1) * 4].reshape(k, depth, a - 1, 4)


@pytest.mark.parametrize("k", PATH_COUNTS)
@pytest.mark.parametrize("label,a,m", PATH_TREES)
def test_the_device_opening_equals_the_host_gather(label, a, m, k):
    leaves, nodes = M.cached_tree(label, a, m)
    depth, _ = M.shape(m, a)
    idx = M.path_indices(m, a, k, seed=k)
    if k >= a + 2:
        assert {0, m - 1} <= set(int(i) for i in idx) and {int(i) % a for i in idx} == set(range(a))
    host = np.zeros((k, depth, a - 1, 4), dtype=np.uint64)
    _lib.check(_lib.lib().pmx_merkle_ary_paths(ctypes.c_void_p(nodes.ctypes.data), m, a, ctypes.c_void_p(idx.ctypes.data), k,
                                               ctypes.c_void_p(host.ctypes.data)))
    assert np.array_equal(host, M.open_paths(nodes, m, a, idx)), "the host gather against the index arithmetic"
    assert np.array_equal(_gather_dev(label, a, m, nodes, idx), host), (label, a, m, k)


def test_the_device_opening_of_an_index_that_names_no_leaf_is_zero():
    leaves, nodes = M.cached_tree("t9-bn254", 8, 512)
    idx = np.array([3, 512, 511, (1 << 64) - 1, 1 << 40], dtype=np.uint64)
    got = _gather_dev("t9-bn254", 8, 512, nodes, idx)
    assert np.array_equal(got[[0, 2]], M.open_paths(nodes, 512, 8, idx[[0, 2]]))
    assert not got[[1, 3, 4]].any()


def test_the_python_tree_opens_and_verifies():
    f, cfg, cr = M.config("t9-bn254")
    leaves, nodes = M.cached_tree("t9-bn254", 8, 512)
    tree = S.MerkleTree(cfg, leaves, arity=8)
    assert np.array_equal(tree.nodes, nodes) and tree.depth == 3 and tree.level_offset(2) == 512 + 64
    idx = M.path_indices(512, 8, 20, seed=5)
    paths = tree.paths(idx)
    assert np.array_equal(paths, M.open_paths(nodes, 512, 8, idx)) and np.array_equal(tree.paths_dev(idx), paths)
    assert np.array_equal(tree.path(77), M.open_paths(nodes, 512, 8, [77])[0])
    ok = S.verify_paths(cfg, leaves[idx.astype(np.int64)], idx, paths, tree.root, arity=8)
    assert ok.all()
    paths[3, 1, 2, 0] ^= np.uint64(1)
    ok = S.verify_paths(cfg, leaves[idx.astype(np.int64)], idx, paths, tree.root, arity=8)
    assert not ok[3] and ok.sum() == 19
    # the defaults are the 2-to-1 tree
    l2, n2 = M.cached_tree("t3", 2, 64)
    t2 = S.MerkleTree(M.config("t3")[1], l2)
    assert t2.arity == 2 and np.array_equal(t2.nodes, n2) and t2.paths([5]).shape == (1, 6, 4)
    assert np.array_equal(t2.paths_dev([5, 63]).reshape(2, 6, 4), t2.paths([5, 63]))
    assert S.verify_paths(M.config("t3")[1], l2[[5]], [5], t2.paths([5]), t2.root).all()


# ---- verification -------------------------------------------------------------------------------------------------------------
def _path_batch(label, a, m, k):
    """k openings of the case's tree: every second path has one limb of one sibling flipped, paths 5, 25, 45, ... carry an index at or
    above arity^depth whose digits still walk a good path (only the range test can fail them).  Expected verdicts from the oracle's climb."""
    f, cfg, cr = M.config(label)
    leaves, nodes = M.cached_tree(label, a, m)
    depth, _ = M.shape(m, a)
    idx = M.path_indices(m, a, k, seed=100 + k)
    paths = M.open_paths(nodes, m, a, idx)
    rng = np.random.default_rng(k)
    corrupt = np.arange(k) % 2 == 1
    for i in np.nonzero(corrupt)[0]:
        paths[i, rng.integers(0, depth), rng.integers(0, a - 1), rng.integers(0, 4)] ^= np.uint64(1) << np.uint64(rng.integers(0, 32))
    high = np.arange(k) % 20 == 4
    idx = idx.copy()
    idx[high] += np.uint64(m) * np.uint64(1 + (k % 3))
    mine = leaves[(idx % np.uint64(m)).astype(np.int64)]
    top = M.climb(cr, mine, idx, paths, a)
    want = ((top == nodes[-1]).all(axis=1) & (idx < np.uint64(m))).astype(np.uint8)
    assert np.array_equal(want, (~corrupt & ~high).astype(np.uint8)), "exactly the corrupted and the out-of-range paths fail"
    return mine, idx, paths, np.array(nodes[-1]), want


@pytest.mark.parametrize("k", PATH_COUNTS)
@pytest.mark.parametrize("label,a,m", PATH_TREES)
def test_batched_verification_fails_exactly_the_bad_paths(label, a, m, k):
    depth, _ = M.shape(m, a)
    mine, idx, paths, root, want = _path_batch(label, a, m, k)
    got = _ctx(label).merkle_ary_verify_paths(mine, idx, paths, depth, a, root)
    assert np.array_equal(got, want), (label, a, m, k)
    assert k == 1 or (got.min(), got.max()) == (0, 1)          # both verdicts occur
    # the same on device-resident buffers; d_ok at an odd address
    d = [_dev(x) for x in (mine, idx, paths, root)]
    d_ok = _dev(np.full(k + 1, 9, dtype=np.uint8))
    d_work = _dev(np.zeros(k * (a + 1) * 4, dtype=np.uint64))
    _ctx(label).merkle_ary_verify_paths_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), depth, a, k, d[3].data_ptr(),
                                            d_ok.data_ptr() + 1, d_work.data_ptr(), _stream())
    ok = _host(d_ok, np.uint8)
    assert ok[0] == 9 and np.array_equal(ok[1:], want)
    if a == 2:      # the verdicts of the 2-to-1 verifier on the same bytes
        old = np.zeros(k, dtype=np.uint8)
        _lib.check(_lib.lib().pmx_merkle_verify_paths(_ctx(label)._h, ctypes.c_void_p(mine.ctypes.data), ctypes.c_void_p(idx.ctypes.data),
                                                      ctypes.c_void_p(paths.ctypes.data), depth, k, ctypes.c_void_p(root.ctypes.data),
                                                      ctypes.c_void_p(old.ctypes.data)))
        assert np.array_equal(old, want)


def test_verification_at_depth_zero_compares_the_leaf_with_the_root():
    leaf, _ = M.cached_tree("t9-bn254", 8, 1)
    other = M.cached_tree("t9-bn254", 8, 512)[0][:1]
    leaves = np.concatenate([leaf, other, leaf])
    idx = np.array([0, 0, 1], dtype=np.uint64)
    got = _ctx("t9-bn254").merkle_ary_verify_paths(leaves, idx, np.zeros((3, 0, 7, 4), dtype=np.uint64), 0, 8, np.array(leaf[0]))
    assert got.tolist() == [1, 0, 0]


# ---- refusals: the status, and nothing written ---------------------------------------------------------------------------------
def test_every_refusal_returns_its_status_and_writes_nothing():
    label, a, m = "t9-bn254", 8, 64
    ctx, L, s = _ctx(label), _lib.lib(), _stream()
    leaves, nodes = M.cached_tree(label, a, m)
    depth, n_nodes = M.shape(m, a)
    sentinel = np.full((n_nodes + 8, 4), 0x1111111111111111, dtype=np.uint64)
    sentinel[:m] = leaves
    d_nodes = _dev(sentinel)
    before = d_nodes.clone()
    h_nodes, h_root = np.full((n_nodes, 4), 3, dtype=np.uint64), np.full(4, 3, dtype=np.uint64)
    k = 5
    idx = M.path_indices(m, a, k, seed=1)
    paths = M.open_paths(nodes, m, a, idx)
    d_leaves, d_idx, d_paths, d_root = _dev(leaves[idx.astype(np.int64)]), _dev(idx), _dev(paths), _dev(np.array(nodes[-1]))
    d_ok, d_work, d_out = _dev(np.full(k, 9, dtype=np.uint8)), _dev(np.full(k * (a + 1) * 4, 4, dtype=np.uint64)), _dev(np.full(paths.shape, 6, dtype=np.uint64))
    outs = [d_ok, d_work, d_out]
    outs_before = [t.clone() for t in outs]
    h_ok = np.full(k, 9, dtype=np.uint8)
    p = lambda t: t.data_ptr()
    v = lambda x: ctypes.c_void_p(x.ctypes.data)

    def calls(arity, n_leaves=m, n_trees=2, dep=depth, nodes_ptr=None):
        """every entry that takes a context, with this arity / shape"""
        dn = p(d_nodes) if nodes_ptr is None else nodes_ptr
        return [
            ("ary", lambda: L.pmx_merkle_ary(ctx._h, v(leaves), n_leaves, arity, v(h_nodes), v(h_root))),
            ("ary_dev", lambda: L.pmx_merkle_ary_dev(ctx._h, dn, n_leaves, arity, s)),
            ("forest", lambda: L.pmx_merkle_ary_forest(ctx._h, v(leaves), n_trees, n_leaves // n_trees if n_leaves >= n_trees else n_leaves, arity, v(h_nodes), v(h_root))),
            ("forest_dev", lambda: L.pmx_merkle_ary_forest_dev(ctx._h, dn, n_trees, n_leaves // n_trees if n_leaves >= n_trees else n_leaves, arity, s)),
            ("paths_dev", lambda: L.pmx_merkle_ary_paths_dev(ctx._h, dn, n_leaves, arity, p(d_idx), k, p(d_out), s)),
            ("verify", lambda: L.pmx_merkle_ary_verify_paths(ctx._h, v(leaves), v(idx), v(paths), dep, arity, k, v(h_root), v(h_ok))),
            ("verify_dev", lambda: L.pmx_merkle_ary_verify_paths_dev(ctx._h, p(d_leaves), p(d_idx), p(d_paths), dep, arity, k, p(d_root), p(d_ok), p(d_work), s)),
        ]

    def untouched():
        torch.cuda.synchronize()
        assert torch.equal(before, d_nodes) and all(torch.equal(x, y) for x, y in zip(outs_before, outs))
        assert (h_nodes == 3).all() and (h_root == 3).all() and (h_ok == 9).all()

    def expect(status, entries, needle=None, only=None):
        for name, call in entries:
            if only and name not in only:
                continue
            assert call() == status, (name, L.pmx_last_error())
            assert needle is None or needle in L.pmx_last_error(), (name, L.pmx_last_error())
            untouched()

    for arity in (0, 1):                                         # arity < 2
        expect(_lib.PMX_ERR_ARG, calls(arity))
    # a leaf count that is no power of the arity (forest: 2 trees of 24 leaves)
    expect(_lib.PMX_ERR_ARG, calls(a, n_leaves=48), only=("ary", "ary_dev", "forest", "forest_dev", "paths_dev"))
    expect(_lib.PMX_ERR_ARG, calls(a, n_leaves=0), only=("ary", "ary_dev", "paths_dev"))
    assert L.pmx_merkle_ary_forest_dev(ctx._h, p(d_nodes), 0, 8, a, s) == _lib.PMX_ERR_ARG      # no trees
    # byte sizes that overflow: 8^20 leaves are 2^65 bytes of nodes; 2^59 trees of 8 leaves
    expect(_lib.PMX_ERR_ARG, calls(a, n_leaves=8 ** 20, n_trees=1), b"overflow", only=("ary", "ary_dev", "forest", "forest_dev", "paths_dev"))
    assert L.pmx_merkle_ary_forest_dev(ctx._h, p(d_nodes), 1 << 59, 8, a, s) == _lib.PMX_ERR_ARG and b"overflow" in L.pmx_last_error()
    assert L.pmx_merkle_ary_forest(ctx._h, v(leaves), 1 << 59, 8, a, v(h_nodes), v(h_root)) == _lib.PMX_ERR_ARG
    untouched()
    # arity^depth beyond 64 bits
    expect(_lib.PMX_ERR_ARG, calls(a, dep=22), b"overflows 64 bits", only=("verify", "verify_dev"))
    expect(_lib.PMX_ERR_ARG, calls(2, dep=64), b"overflows 64 bits", only=("verify", "verify_dev"))
    # null pointers
    assert L.pmx_merkle_ary(None, v(leaves), m, a, v(h_nodes), v(h_root)) == _lib.PMX_ERR_ARG
    assert L.pmx_merkle_ary(ctx._h, None, m, a, v(h_nodes), v(h_root)) == _lib.PMX_ERR_ARG
    assert L.pmx_merkle_ary_dev(ctx._h, None, m, a, s) == _lib.PMX_ERR_ARG
    assert L.pmx_merkle_ary_dev(None, p(d_nodes), m, a, s) == _lib.PMX_ERR_ARG
    assert L.pmx_merkle_ary_forest(ctx._h, None, 1, m, a, v(h_nodes), v(h_root)) == _lib.PMX_ERR_ARG
    assert L.pmx_merkle_ary_forest_dev(ctx._h, None, 1, m, a, s) == _lib.PMX_ERR_ARG
    for hole in range(3):
        args = [p(d_nodes), p(d_idx), p(d_out)]
        args[hole] = None
        assert L.pmx_merkle_ary_paths_dev(ctx._h, args[0], m, a, args[1], k, args[2], s) == _lib.PMX_ERR_ARG, hole
    assert L.pmx_merkle_ary_paths_dev(None, p(d_nodes), m, a, p(d_idx), k, p(d_out), s) == _lib.PMX_ERR_ARG
    for hole in range(6):
        args = [p(d_leaves), p(d_idx), p(d_paths), p(d_root), p(d_ok), p(d_work)]
        args[hole] = None
        assert L.pmx_merkle_ary_verify_paths_dev(ctx._h, args[0], args[1], args[2], depth, a, k, args[3], args[4], args[5], s) == _lib.PMX_ERR_ARG, hole
    for hole in range(5):
        args = [v(leaves), v(idx), v(paths), v(h_root), v(h_ok)]
        args[hole] = None
        assert L.pmx_merkle_ary_verify_paths(ctx._h, args[0], args[1], args[2], depth, a, k, args[3], args[4]) == _lib.PMX_ERR_ARG, hole
    untouched()
    # an element array that is not 16-byte aligned
    expect(_lib.PMX_ERR_ARG, calls(a, n_trees=1, nodes_ptr=p(d_nodes) + 8), b"16-byte aligned", only=("ary_dev", "forest_dev", "paths_dev"))
    # arity beyond the rate: a configuration error that points at the hash driver (rate 3 here; arity 4 of 64 leaves is a good shape)
    ctx4 = _ctx("t4")
    big = [
        lambda: L.pmx_merkle_ary(ctx4._h, v(leaves), 64, 4, v(h_nodes), v(h_root)),
        lambda: L.pmx_merkle_ary_dev(ctx4._h, p(d_nodes), 64, 4, s),
        lambda: L.pmx_merkle_ary_forest(ctx4._h, v(leaves), 4, 16, 4, v(h_nodes), v(h_root)),
        lambda: L.pmx_merkle_ary_forest_dev(ctx4._h, p(d_nodes), 4, 16, 4, s),
        lambda: L.pmx_merkle_ary_paths_dev(ctx4._h, p(d_nodes), 64, 4, p(d_idx), k, p(d_out), s),
        lambda: L.pmx_merkle_ary_verify_paths(ctx4._h, v(leaves), v(idx), v(paths), 2, 4, k, v(h_root), v(h_ok)),
        lambda: L.pmx_merkle_ary_verify_paths_dev(ctx4._h, p(d_leaves), p(d_idx), p(d_paths), 2, 4, k, p(d_root), p(d_ok), p(d_work), s),
    ]
    for n, call in enumerate(big):
        assert call() == _lib.PMX_ERR_CONFIG, (n, L.pmx_last_error())
        assert b"pmx_hash_batch_dev" in L.pmx_last_error() and b"rate" in L.pmx_last_error()
        untouched()
    # and the context still builds the right tree
    got, _ = ctx.merkle_ary(leaves, a)
    assert np.array_equal(got, nodes)
