"""Trees of a fixed depth through the C ABI (pmx_merkle_fixed_defaults, pmx_merkle_frontier_append, pmx_merkle_fixed,
pmx_merkle_fixed_paths) on every engine that serves them.  Expected values never come from the product: tests/merkle_fixed_oracle.py
pads the leaf row with the default leaf to arity^depth leaves and hashes every level with the C port; for depths nobody can pad it hashes
the populated part over the default chain (tests/test_merkle_fixed_host.py asserts that the two agree).

One refusal the issue's list does not name: a FULL tree's frontier holds no node, so n_leaves = arity^depth with m = 0 cannot return a
root; the call is PMX_ERR_ARG unless root is NULL (include/poseidon_mi355x.h says so), and the exhaustive append test asserts exactly that
for its one such (n, m)."""
import ctypes

import numpy as np
import pytest

import sponge_amd as S
from sponge_amd import _lib
from sponge_amd.poseidon import merkle_fixed_paths

import merkle_fixed_oracle as M

pytestmark = pytest.mark.gpu

GARBAGE = 0xDEADBEEFDEADBEEF
SMALL = [("t3", 2, 4), ("t9-bn254", 3, 3)]
DENSE = [("t3", 2, 4, list(range(1, 17))), ("t9-bn254", 3, 3, list(range(1, 28))), ("t9-bn254", 8, 2, [1, 7, 8, 9, 63, 64])]


def _ctx(label):
    return M.config(label)[1].context()


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _engine(label, parents, arity):
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(_ctx(label)._h, _lib.OP_COMPRESS, parents, arity, ctypes.byref(info)))
    return info.engine


def _dirty(frontier, n, a):
    """the frontier with garbage in the slots at or beyond the digit: ignored on input"""
    out = frontier.copy()
    for l in range(out.shape[0]):
        out[l, (n // a ** l) % a:] = GARBAGE
    return out


# ---- defaults -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,a,depth", [("t3", 2, 32), ("t9-bn254", 8, 21), ("t9-bn254", 2, 64), ("t5", 4, 16)])
def test_defaults_are_the_oracle_chain(label, a, depth):
    want = M.cached_defaults(label, a, depth)
    got = _ctx(label).merkle_fixed_defaults(M.default_leaf(label), a, depth)
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], M.default_leaf(label))


# ---- the dense tree -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,a,depth,counts", DENSE)
def test_every_node_of_the_dense_tree_equals_the_oracle(label, a, depth, counts):
    e = M.cached_defaults(label, a, depth)
    row = M.leaf_row(label, a ** depth)
    for n in counts:
        levels = M.cached_padded(label, a, depth, n)
        nodes, root = _ctx(label).merkle_fixed(row[:n], a, depth, e)
        assert np.array_equal(nodes, M.dense_of(levels, n, a, depth)), (label, a, depth, n)
        assert np.array_equal(root, levels[depth][0])
        _, only_root = _ctx(label).merkle_fixed(row[:n], a, depth, e, want_nodes=False)
        assert np.array_equal(only_root, root)
        # the root of pmx_merkle_ary over the explicitly padded row
        _, ary_root = _ctx(label).merkle_ary(levels[0], a)
        assert root.tobytes() == ary_root.tobytes()
    full, _ = _ctx(label).merkle_fixed(row, a, depth, e)
    ary, _ = _ctx(label).merkle_ary(row, a)
    assert full.tobytes() == ary.tobytes()                       # at n = a^depth: byte for byte the array of pmx_merkle_ary


# ---- append ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,a,depth", SMALL)
def test_every_append_gives_the_oracles_frontier_and_root(label, a, depth):
    ctx, e, cap = _ctx(label), M.cached_defaults(label, a, depth), a ** depth
    row = M.leaf_row(label, cap)
    lib = _lib.lib()
    for n in range(cap + 1):
        before = M.frontier_of(M.cached_padded(label, a, depth, n), n, a, depth)
        for m in range(cap - n + 1):
            after = M.cached_padded(label, a, depth, n + m)
            want = M.frontier_of(after, n + m, a, depth)
            full_and_nothing = n == cap and m == 0                 # no frontier node at all: the root cannot be recomputed
            got, root = ctx.merkle_frontier_append(a, depth, e, _dirty(before, n, a), n, row[n:n + m], want_root=not full_and_nothing)
            assert got.tobytes() == want.tobytes(), (label, n, m)    # unused slots zero, garbage in unused input slots ignored
            if full_and_nothing:
                out = np.full((depth, a - 1, 4), 0x77, dtype=np.uint64)
                top = np.full(4, 0x77, dtype=np.uint64)
                assert lib.pmx_merkle_frontier_append(ctx._h, a, depth, _p(np.ascontiguousarray(e)), _p(before), n, None, 0, _p(out),
                                                      _p(top)) == _lib.PMX_ERR_ARG
                assert (out == 0x77).all() and (top == 0x77).all()
            else:
                assert np.array_equal(root, after[depth][0]), (label, n, m)
            if m in (0, 1, cap - n) and not full_and_nothing:        # frontier_out aliasing frontier_in
                io, top = _dirty(before, n, a), np.zeros(4, dtype=np.uint64)
                _lib.check(lib.pmx_merkle_frontier_append(ctx._h, a, depth, _p(np.ascontiguousarray(e)), _p(io), n, _p(np.ascontiguousarray(row[n:n + m])) if m else None,
                                                          m, _p(io), _p(top)))
                assert io.tobytes() == want.tobytes() and np.array_equal(top, after[depth][0])
    # NULL frontier_in at n = 0
    got, root = ctx.merkle_frontier_append(a, depth, e, None, 0, row[:5])
    assert np.array_equal(got, M.frontier_of(M.cached_padded(label, a, depth, 5), 5, a, depth))


@pytest.mark.parametrize("label,a,depth", SMALL)
def test_split_invariance(label, a, depth):
    ctx, e, cap = _ctx(label), M.cached_defaults(label, a, depth), a ** depth
    row = M.leaf_row(label, cap)
    whole, whole_root = ctx.merkle_frontier_append(a, depth, e, None, 0, row)
    assert np.array_equal(whole_root, M.cached_padded(label, a, depth, cap)[depth][0]) and not whole.any()
    for first in range(cap + 1):
        f1, r1 = ctx.merkle_frontier_append(a, depth, e, None, 0, row[:first])
        f2, r2 = ctx.merkle_frontier_append(a, depth, e, f1, first, row[first:], want_root=first < cap)
        assert f2.tobytes() == whole.tobytes() and (first == cap or r2.tobytes() == whole_root.tobytes())
        if first == cap:
            assert r1.tobytes() == whole_root.tobytes()


def test_more_leaves_than_positions_is_refused_and_writes_nothing():
    label, a, depth = "t3", 2, 4
    ctx, e = _ctx(label), np.ascontiguousarray(M.cached_defaults(label, a, depth))
    row = np.ascontiguousarray(M.leaf_row(label, 17))
    out, top = np.full((depth, a - 1, 4), 0x77, dtype=np.uint64), np.full(4, 0x77, dtype=np.uint64)
    for n, m in ((0, 17), (16, 1), (9, 8)):
        before = np.ascontiguousarray(M.frontier_of(M.cached_padded(label, a, depth, n), n, a, depth))
        assert _lib.lib().pmx_merkle_frontier_append(ctx._h, a, depth, _p(e), _p(before), n, _p(row), m, _p(out), _p(top)) == _lib.PMX_ERR_ARG
        assert (out == 0x77).all() and (top == 0x77).all()
    # the errors that need the context: more children than the rate
    assert _lib.lib().pmx_merkle_frontier_append(ctx._h, 3, depth, _p(e), None, 0, _p(row), 2, _p(out), _p(top)) == _lib.PMX_ERR_CONFIG
    assert _lib.lib().pmx_merkle_fixed_defaults(ctx._h, _p(row), 3, depth, _p(out)) == _lib.PMX_ERR_CONFIG
    assert _lib.lib().pmx_merkle_fixed(ctx._h, _p(row), 2, 3, depth, _p(e), _p(out), _p(top)) == _lib.PMX_ERR_CONFIG
    assert (out == 0x77).all() and (top == 0x77).all()


@pytest.mark.parametrize("label,a,depth", [("t3", 2, 32), ("t9-bn254", 8, 21)])
def test_carries_at_every_power_of_the_arity(label, a, depth):
    """n = a^j - 1 identical leaves x, one more appended, for every j <= depth.  Every complete node of level l of such a tree is c[l], the
    chain of x, so the frontier of a^j - 1 leaves is a - 1 copies of c[l] below level j; afterwards it is one c[j] at level j, and the
    root is c[j] hashed up with default digests to its right (j = depth: the root is c[depth], a complete node)."""
    f, _, cr = M.config(label)
    ctx, e = _ctx(label), M.cached_defaults(label, a, depth)
    x = M.leaf_row(label, 1, seed=7)[0]
    c = M.defaults(cr, x, a, depth)
    for j in range(depth + 1):
        before = np.zeros((depth, a - 1, 4), dtype=np.uint64)
        for l in range(j):
            before[l, :] = c[l]
        want = np.zeros((depth, a - 1, 4), dtype=np.uint64)
        if j < depth:
            want[j, 0] = c[j]
        top = c[j]
        for l in range(j, depth):
            top = cr.hash_batch(np.concatenate([top.reshape(1, 4), np.repeat(e[l].reshape(1, 4), a - 1, axis=0)]).reshape(1, a, 4), a, 1, threads=1).reshape(4)
        got, root = ctx.merkle_frontier_append(a, depth, e, before, a ** j - 1, x.reshape(1, 4))
        assert got.tobytes() == want.tobytes() and np.array_equal(root, top), (label, j)


def test_filling_the_whole_tree_in_one_append():
    label, a, depth = "t3", 2, 10
    e, row = M.cached_defaults(label, a, depth), M.leaf_row(label, 1 << 10)
    levels = M.cached_padded(label, a, depth, 1 << 10)
    got, root = _ctx(label).merkle_frontier_append(a, depth, e, None, 0, row)
    assert not got.any() and np.array_equal(root, levels[depth][0])       # the root is a complete node, no partial node exists
    _, ary_root = _ctx(label).merkle_ary(row, a)
    assert root.tobytes() == ary_root.tobytes()


# ---- deep trees, engines, pieces ------------------------------------------------------------------------------------------
def _deep(label, a, depth, n, m):
    """(frontier before, frontier after, root after) off the populated part"""
    _, _, cr = M.config(label)
    e, row = M.cached_defaults(label, a, depth), M.leaf_row(label, n + m)
    before = M.frontier_of(M.sparse_levels(cr, row[:n], a, depth, e), n, a, depth)
    levels = M.sparse_levels(cr, row, a, depth, e)
    return before, M.frontier_of(levels, n + m, a, depth), M.root_of(levels, e, depth)


def _parents(n, m, a, depth):
    out = []
    for l in range(depth):
        f, g = n // a ** l, (n + m) // a ** l
        out.append(-(-(f % a + g - f + (1 if (n + m) % a ** l else 0)) // a))
    return out


@pytest.mark.parametrize("label,a,depth", [("t3", 2, 32), ("t9-bn254", 8, 21)])
def test_deep_trees(label, a, depth):
    before, want, want_root = _deep(label, a, depth, 1000, 300)
    got, root = _ctx(label).merkle_frontier_append(a, depth, M.cached_defaults(label, a, depth), before, 1000, M.leaf_row(label, 1300)[1000:])
    assert got.tobytes() == want.tobytes() and np.array_equal(root, want_root)


@pytest.mark.parametrize("label,a,depth,m,engines", [
    ("t3", 2, 32, 257, [b"QuadEngine<5>"]),
    ("t3", 2, 32, 2 * 32768 + 2, [b"HybridEngine<3,5", b"QuadEngine<5>"]),          # 32769 parents: the window engine, then the latency engine
    ("t9-bn254", 8, 21, 300, [b"HybridEngine<9,5"]),
    ("t9-bn254", 2, 32, 300, [b"HybridEngine<9,5"]),
    ("t10", 9, 8, 300, [b"LdsEngine<5>"]),
])
def test_every_level_runs_on_the_engine_the_context_names(label, a, depth, m, engines):
    parents = _parents(0, m, a, depth)
    for l, count in enumerate(parents):
        assert _engine(label, count, a).startswith(engines[min(l, len(engines) - 1)]), (l, count, _engine(label, count, a))
    _, want, want_root = _deep(label, a, depth, 0, m)
    e = _ctx(label).merkle_fixed_defaults(M.default_leaf(label), a, depth)
    assert np.array_equal(e, M.cached_defaults(label, a, depth))
    got, root = _ctx(label).merkle_frontier_append(a, depth, e, None, 0, M.leaf_row(label, m))
    assert got.tobytes() == want.tobytes() and np.array_equal(root, want_root)


def _bind(handle, name):
    fn = getattr(handle, name)
    fn.restype, fn.argtypes = (_lib.SIGNATURES.get(name) or _lib.TEST_HOOK_SIGNATURES[name])
    return fn


def test_pieces_change_no_byte():
    """pieces of 64 leaves (the test library's hook): m = 1000 behind n = 1000 at (2, 32), 16 pieces with a short last one, then 143 pieces of 7, and the dense
    tree over 1000 leaves, against the calls in one piece and against the session's library"""
    label, a, depth, n, m = "t3", 2, 32, 1000, 1000
    _, cfg, _ = M.config(label)
    e = np.ascontiguousarray(M.cached_defaults(label, a, depth))
    row = np.ascontiguousarray(M.leaf_row(label, n + m))
    before, want, want_root = _deep(label, a, depth, n, m)
    before = np.ascontiguousarray(before)
    session, session_root = _ctx(label).merkle_frontier_append(a, depth, e, before, n, row[n:])
    assert session.tobytes() == want.tobytes() and np.array_equal(session_root, want_root)
    dense_want, dense_root = _ctx(label).merkle_fixed(row[:n], a, depth, e)
    handle = ctypes.CDLL(_lib.TEST_LIB_PATH)
    c, h = S.poseidon.c_config(cfg), ctypes.c_void_p()
    assert _bind(handle, "pmx_ctx_create")(ctypes.byref(c), 0, ctypes.byref(h)) == _lib.PMX_OK
    try:
        for piece in (0, 64, 7):
            assert _bind(handle, "pmx_test_merkle_fixed_piece")(piece) == _lib.PMX_OK
            out, top = np.zeros_like(want), np.zeros(4, dtype=np.uint64)
            assert _bind(handle, "pmx_merkle_frontier_append")(h, a, depth, _p(e), _p(before), n, _p(row[n:]), m, _p(out), _p(top)) == _lib.PMX_OK
            assert out.tobytes() == want.tobytes() and np.array_equal(top, want_root), piece
            nodes = np.zeros_like(dense_want)
            assert _bind(handle, "pmx_merkle_fixed")(h, _p(row), n, a, depth, _p(e), _p(nodes), _p(top)) == _lib.PMX_OK
            assert nodes.tobytes() == dense_want.tobytes() and np.array_equal(top, dense_root), piece
    finally:
        _bind(handle, "pmx_test_merkle_fixed_piece")(0)
        _bind(handle, "pmx_ctx_destroy")(h)


# ---- paths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,a,depth,counts", DENSE)
def test_every_opening_verifies_through_the_existing_verifier(label, a, depth, counts):
    ctx, e = _ctx(label), M.cached_defaults(label, a, depth)
    row = M.leaf_row(label, a ** depth)
    for n in counts:
        nodes, root = ctx.merkle_fixed(row[:n], a, depth, e)
        idx = np.arange(n, dtype=np.uint64)
        paths = merkle_fixed_paths(nodes, n, a, depth, e, idx)
        assert np.array_equal(paths, M.open_paths(M.cached_padded(label, a, depth, n), n, a, depth, e, idx))
        assert ctx.merkle_ary_verify_paths(np.ascontiguousarray(row[:n]), idx, paths, depth, a, root).all(), (label, n)
        bad = paths.copy()
        bad[n // 2, depth - 1, 0, 3] ^= np.uint64(1 << 17)          # one flipped bit in the top sibling of one path
        ok = ctx.merkle_ary_verify_paths(np.ascontiguousarray(row[:n]), idx, bad, depth, a, root)
        assert not ok[n // 2] and ok.sum() == n - 1
        out = np.full((2, depth, a - 1, 4), 0x55, dtype=np.uint64)
        bad_idx = np.array([0, n], dtype=np.uint64)
        assert _lib.lib().pmx_merkle_fixed_paths(_p(nodes), n, a, depth, _p(np.ascontiguousarray(e)), _p(bad_idx), 2, _p(out)) == _lib.PMX_ERR_ARG
        assert (out == 0x55).all()


# ---- Python ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,a,depth", [("t3", 2, 32), ("t9-bn254", 8, 21)])
def test_incremental_tree_in_three_batches_has_the_root_of_the_dense_tree(label, a, depth):
    _, cfg, _ = M.config(label)
    row = M.leaf_row(label, 700)
    tree = S.IncrementalMerkleTree(cfg, depth, arity=a, default_leaf=M.default_leaf(label))
    assert np.array_equal(tree.root, M.cached_defaults(label, a, depth)[depth]) and tree.n_leaves == 0
    for lo, hi in ((0, 1), (1, 450), (450, 700)):
        tree.append(row[lo:hi])
    dense = S.MerkleTree.fixed(cfg, row, depth, a, M.default_leaf(label))
    assert tree.n_leaves == 700 and tree.root.tobytes() == dense.root.tobytes()
    assert np.array_equal(tree.defaults, dense.defaults)
    _, want, want_root = _deep(label, a, depth, 0, 700)
    assert tree.frontier.tobytes() == want.tobytes() and np.array_equal(tree.root, want_root)
    paths = dense.open([0, 699, 350])
    assert cfg.context().merkle_ary_verify_paths(np.ascontiguousarray(row[[0, 699, 350]]), np.array([0, 699, 350], dtype=np.uint64), paths, depth, a,
                                                 dense.root).all()
    zero = S.IncrementalMerkleTree(cfg, depth, arity=a)           # the default default leaf is the field's zero
    assert not zero.defaults[0].any()
