"""Sequential leaf updates of a fixed-depth tree with witnesses through the C ABI (pmx_merkle_update_witnesses) on the engines that serve
its level launches.  Expected values never come from the product:
- small dense trees: the C port's tree (tests/merkle_ary_oracle.py) rebuilt after every single update - witness[j] is its opening of
  indices[j] after j updates, roots[j] its root after update j -, and every witness climbs, through the existing
  pmx_merkle_ary_verify_paths, with the old leaf to roots[j - 1] and with the new leaf to roots[j];
- deep sparse trees nobody can pad (2^32, 2^64, 8^21 positions): the overlay model of tests/merkle_chain_oracle.py over old openings the
  oracle builds from the chain of default digests;
- more than 32768 updates at t = 3 (the level launch on the window engine): the model hashed level by level by the C port.
PMX_ERR_CONFIG for arity > rate, the one refusal that reads a context, is here too."""
import ctypes
import functools

import numpy as np
import pytest

import sponge_amd as S
from sponge_amd import _lib, synth

import merkle_ary_oracle as MA
import merkle_chain_oracle as C
import merkle_fixed_oracle as MF

pytestmark = pytest.mark.gpu

# (label, arity, depth); "t3" is BLS12-381 at t = 3, whose 2-to-1 launches up to 32768 rows run on the quad engine
DENSE = [("t9-bn254", 2, 4), ("t5", 4, 3), ("t9-bn254", 8, 2), ("t9-bn254", 3, 3), ("t3", 2, 4)]
COUNTS = [1, 2, 65, 200]


def _ctx(label):
    return MA.config(label)[1].context()


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _engine(label, rows, arity):
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(_ctx(label)._h, _lib.OP_COMPRESS, rows, arity, ctypes.byref(info)))
    return info.engine


@functools.lru_cache(maxsize=None)
def dense_case(label, a, depth, k):
    """(indices, new leaves, old leaves, old openings, old root, witnesses, roots) of k updates of the dense tree of a case, by k rebuilds:
    the indices come from a few leaves and from anywhere by turns, so ancestors are shared and indices repeat; read-only"""
    f, _, cr = MA.config(label)
    n = a ** depth
    leaves, nodes = MA.cached_tree(label, a, n)
    rng = np.random.default_rng(1000 * a + 10 * depth + k)
    idx = np.array([int(rng.integers(0, min(n, 2 * a + 1))) if j % 2 == 0 else int(rng.integers(0, n)) for j in range(k)], dtype=np.uint64)
    if k == 2:
        idx[1] = idx[0] ^ np.uint64(1)                       # two children of one parent
    new = synth.random_elements(f, k, seed=0x51 + k)
    paths = MA.open_paths(nodes, n, a, idx)
    row, tree = np.array(leaves), nodes
    old = np.zeros((k, 4), dtype=np.uint64)
    witness = np.zeros((k, depth, a - 1, 4), dtype=np.uint64)
    roots = np.zeros((k, 4), dtype=np.uint64)
    for j, i in enumerate(int(x) for x in idx):
        witness[j] = MA.open_paths(tree, n, a, [i])[0]
        old[j] = row[i]
        row[i] = new[j]
        tree = MA.tree(cr, row, a)
        roots[j] = tree[-1]
    out = (idx, new, old, paths, np.array(nodes[-1]), witness, roots)
    for x in out:
        x.setflags(write=False)
    return out


@pytest.mark.parametrize("k", COUNTS)
@pytest.mark.parametrize("label,a,depth", DENSE)
def test_witnesses_and_roots_are_the_tree_rebuilt_after_every_update(label, a, depth, k):
    idx, new, old, paths, old_root, want_w, want_r = dense_case(label, a, depth, k)
    if label == "t3":
        assert _engine(label, k, a).startswith(b"QuadEngine<5>")
    ctx = _ctx(label)
    wit, roots, root = ctx.merkle_update_witnesses(a, depth, idx, new, paths, want_root=True)
    assert wit.tobytes() == want_w.tobytes()
    assert roots.tobytes() == want_r.tobytes()
    assert root.tobytes() == want_r[-1].tobytes()
    # every witness opens the old leaf in the tree before its update and the new leaf in the tree after it
    for j in range(k):
        before = old_root if j == 0 else roots[j - 1]
        assert ctx.merkle_ary_verify_paths(old[j:j + 1], idx[j:j + 1], wit[j:j + 1], depth, a, before)[0] == 1, j
        assert ctx.merkle_ary_verify_paths(new[j:j + 1], idx[j:j + 1], wit[j:j + 1], depth, a, roots[j])[0] == 1, j
    w2, r2 = S.update_witnesses(MA.config(label)[1], depth, idx, new, paths, arity=a)
    assert np.array_equal(w2, wit) and np.array_equal(r2, roots)


@pytest.mark.parametrize("label,a,depth", [("t5", 4, 3), ("t3", 2, 4)])
def test_null_outputs_leave_the_other_outputs_bytes_unchanged(label, a, depth):
    idx, new, _, paths, _, want_w, want_r = dense_case(label, a, depth, 65)
    ctx = _ctx(label)
    for ww in (False, True):
        for wr in (False, True):
            for wt in (False, True):
                wit, roots, root = ctx.merkle_update_witnesses(a, depth, idx, new, paths, want_witnesses=ww, want_roots=wr, want_root=wt)
                assert (wit is None) == (not ww) and (roots is None) == (not wr) and (root is None) == (not wt)
                assert wit is None or wit.tobytes() == want_w.tobytes()
                assert roots is None or roots.tobytes() == want_r.tobytes()
                assert root is None or root.tobytes() == want_r[-1].tobytes()


def _deep_indices(a, depth):
    """64 indices: the ends of the tree, the two sides of its middle, adjacent leaves, children of one parent, one index three times"""
    cap = a ** depth
    half = cap // 2
    rng = np.random.default_rng(a * depth)
    idx = [0, half, cap - 1, half - 1, 1, cap - 2, 1000, 1001, 1002, 7, 1000, half + 5, 1000, 0, cap - 1]
    idx += [a * 12345 + c for c in range(a)]
    while len(idx) < 64:
        idx.append(int(rng.integers(0, 1 << 62)) * 4 % cap if len(idx) % 3 else idx[int(rng.integers(0, len(idx)))] ^ 1)
    return np.array(idx[:64], dtype=np.uint64)


@pytest.mark.parametrize("label,a,depth", [("t3", 2, 32), ("t3", 2, 64), ("t9-bn254", 8, 21)])
def test_deep_sparse_trees_follow_the_overlay_model(label, a, depth):
    f, _, cr = MA.config(label)
    ctx = _ctx(label)
    e = ctx.merkle_fixed_defaults(MF.default_leaf(label), a, depth)
    idx = _deep_indices(a, depth)
    assert {0, a ** depth // 2, a ** depth - 1} <= {int(x) for x in idx} and list(idx).count(1000) == 3
    new = synth.random_elements(f, 64, seed=0xDEE9)
    # the old tree: a handful of leaves set, some of them updated below, some next to updated ones; every other position the default leaf
    held = synth.random_elements(f, 6, seed=0x01D)
    old_leaves = {0: held[0], 1001: held[1], 1003: held[2], a ** depth - 1: held[3], a ** depth // 2 + 4: held[4], 5: held[5]}
    old = C.sparse_tree(cr, a, depth, e, old_leaves)
    paths = C.sparse_paths(old, a, depth, e, idx)
    want_w, want_r = C.model(cr, a, depth, idx, new, paths)
    wit, roots, root = ctx.merkle_update_witnesses(a, depth, idx, new, paths, want_root=True)
    assert wit.tobytes() == want_w.tobytes()
    assert roots.tobytes() == want_r.tobytes() and root.tobytes() == want_r[-1].tobytes()
    # (the oracle's own cross-check: the last root is the root of the sparse tree over the leaves as they end)
    final = dict(old_leaves)
    final.update({int(i): new[j] for j, i in enumerate(idx)})
    assert np.array_equal(C.sparse_root(C.sparse_tree(cr, a, depth, e, final), e, depth), want_r[-1])
    # the first witness is the old opening; it climbs from the old leaf to the old root through the existing verifier
    first = old_leaves.get(int(idx[0]), e[0]).reshape(1, 4)
    assert np.array_equal(wit[0], paths[0])
    if depth < 64:      # (pmx_merkle_ary_verify_paths takes a^depth as a 64-bit limit)
        assert ctx.merkle_ary_verify_paths(np.ascontiguousarray(first), idx[:1], wit[:1], depth, a, C.sparse_root(old, e, depth))[0] == 1


def test_a_level_of_more_than_32768_rows_runs_on_the_window_engine():
    label, a, depth, k = "t3", 2, 2, 32768 + 3
    assert _engine(label, 32768, a).startswith(b"QuadEngine<5>") and _engine(label, k, a).startswith(b"HybridEngine<3,5")
    f, _, cr = MA.config(label)
    leaves, nodes = MA.cached_tree(label, a, 4)
    rng = np.random.default_rng(32771)
    idx = rng.integers(0, 4, k).astype(np.uint64)
    new = synth.random_elements(f, k, seed=0x817)
    paths = MA.open_paths(nodes, 4, a, idx)
    want_w, want_r = C.model_batched(cr, a, depth, idx, new, paths)
    wit, roots, root = _ctx(label).merkle_update_witnesses(a, depth, idx, new, paths, want_root=True)
    assert wit.tobytes() == want_w.tobytes()
    assert roots.tobytes() == want_r.tobytes() and root.tobytes() == want_r[-1].tobytes()
    # the root after the last update is the root of the four leaves as they end
    row = np.array(leaves)
    for j in range(k):
        row[int(idx[j])] = new[j]
    assert np.array_equal(MA.tree(cr, row, a)[-1], root)


def test_refusals_that_read_the_context_write_nothing():
    lib = _lib.lib()
    ctx = _ctx("t3")                                            # rate 2
    idx = np.array([1, 2], dtype=np.uint64)
    buf = np.zeros((2 * 4 * 2, 4), dtype=np.uint64)
    wit = np.full((2, 4, 2, 4), 0x77, dtype=np.uint64)
    roots = np.full((2, 4), 0x77, dtype=np.uint64)
    root = np.full(4, 0x77, dtype=np.uint64)
    assert lib.pmx_merkle_update_witnesses(ctx._h, 3, 4, _p(idx), _p(buf), _p(buf), 2, _p(wit), _p(roots), _p(root)) == _lib.PMX_ERR_CONFIG
    assert b"exceeds the rate" in lib.pmx_last_error()
    assert (wit == 0x77).all() and (roots == 0x77).all() and (root == 0x77).all()
    # k = 0 on a real context: PMX_OK without a root, PMX_ERR_ARG with one
    assert lib.pmx_merkle_update_witnesses(ctx._h, 2, 4, None, None, None, 0, _p(wit), _p(roots), None) == _lib.PMX_OK
    assert lib.pmx_merkle_update_witnesses(ctx._h, 2, 4, None, None, None, 0, None, None, _p(root)) == _lib.PMX_ERR_ARG
    assert (wit == 0x77).all() and (roots == 0x77).all() and (root == 0x77).all()
