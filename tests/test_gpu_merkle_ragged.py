"""Merkle trees over any number of leaves, their openings, path verification and leaf updates through the C ABI (pmx_merkle_ragged*), on
every engine that serves them.  Expected values never come from the product: node arrays are the C port applied level by level with
the short parent as an absorb of the children that exist (tests/merkle_ragged_oracle.py), and tests/golden/merkle_ragged_vectors.json
pins two trees from the Python big-integer oracle.

Shapes are the smallest that reach each way a short row can go wrong (levels as widths):
  t9-bn254  8  1024   128, 16, 2, 1          a power of two that is no power of 8; top parent of 2
  t9-bn254  8  2048   256, 32, 4, 1          top parent of 4; one full workgroup
  t9-bn254  8  513    65, 9, 2, 1            r = 1 three levels running; the short parent is lane 0 of a second wave
  t9-bn254  8  511    64, 8, 1               r = 7; the short parent is the last lane of a full wave
  t9-bn254  8  4097   513, 65, 9, 2, 1       the short parent beyond the first workgroup
  t9-alpha17 8 100    13, 2, 1               generic S-box, r = 4 then 5
  t4        3  100    34, 12, 4, 2, 1        arity = rate, r = 1 on three levels
  t6        4  1000   250, 63, 16, 4, 1      arity below the rate; r = 2, then r = 3
  lds-t16   15 226    16, 2, 1               run-time width, r = 1 twice
  lds-t16   7  300    43, 7, 1               run-time width, r = 6
  t3        2  100    50, 25, 13, 7, 4, 2, 1 quad engine, odd levels
  t3        2  65539  32770, ...             the window engine at t = 3 (above 32768 parents) with r = 1
and, for three labels, 1, 2, a and a + 1 leaves: no launch; a single short parent; a full one; full + r = 1."""
import ctypes

import numpy as np
import pytest
import torch

import sponge_amd as S
from sponge_amd import _lib, synth
from oracle import cref

import merkle_ary_oracle as MA
import merkle_ragged_oracle as M
from helpers import FIELDS, golden

pytestmark = pytest.mark.gpu

# (label, arity, leaves, levels above the leaves)
TABLE = [
    ("t9-bn254", 8, 1024, [128, 16, 2, 1]),
    ("t9-bn254", 8, 2048, [256, 32, 4, 1]),
    ("t9-bn254", 8, 513, [65, 9, 2, 1]),
    ("t9-bn254", 8, 511, [64, 8, 1]),
    ("t9-bn254", 8, 4097, [513, 65, 9, 2, 1]),
    ("t9-alpha17", 8, 100, [13, 2, 1]),
    ("t4", 3, 100, [34, 12, 4, 2, 1]),
    ("t6", 4, 1000, [250, 63, 16, 4, 1]),
    ("lds-t16", 15, 226, [16, 2, 1]),
    ("lds-t16", 7, 300, [43, 7, 1]),
    ("t3", 2, 100, [50, 25, 13, 7, 4, 2, 1]),
    ("t3", 2, 65539, [32770, 16385, 8193, 4097, 2049, 1025, 513, 257, 129, 65, 33, 17, 9, 5, 3, 2, 1]),
]
TREES = [(label, a, m) for label, a, m, _ in TABLE] + \
        [(label, a, m) for label, a in (("t9-bn254", 8), ("t3", 2), ("lds-t16", 15)) for m in (1, 2, a, a + 1)]
ENGINE = {"t4": b"HybridEngine<4,5", "t6": b"HybridEngine<6,5", "t9-bn254": b"HybridEngine<9,5", "t9-alpha17": b"HybridEngine<9,0",
          "lds-t16": b"LdsEngine<5>", "t3": b"QuadEngine<5>"}
POWERS = [("t9-bn254", 8, 512), ("t4", 3, 81), ("t3", 2, 64)]
PATH_TREES = [("t9-bn254", 8, 513), ("t9-bn254", 8, 1024), ("t4", 3, 100), ("t6", 4, 1000), ("lds-t16", 15, 226), ("t3", 2, 100)]
PATH_COUNTS = [1, 65, 257]
UPDATE_TREES = [("t9-bn254", 8, 513, (1, 3, 64, 70)), ("t6", 4, 1000, (1, 3, 64, 260)), ("t3", 2, 100, (1, 3, 64, 100))]
U64 = (1 << 64) - 1
FILL = 0x5A5A5A5A5A5A5A5A


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


def _void(a):
    return ctypes.c_void_p(a.ctypes.data)


def _engine(label, n, length):
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(_ctx(label)._h, _lib.OP_COMPRESS, n, length, ctypes.byref(info)))
    return info


def test_the_table_is_the_arithmetic():
    for label, a, m, levels in TABLE:
        assert M.widths(m, a)[1:] == levels and M.CONFIGS[label][1] >= a
        assert any(w % a for w in M.widths(m, a)[:-1]), "every case has a short row"


# ---- every node -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,a,m", TREES)
def test_every_node_of_the_tree_equals_the_oracle(label, a, m):
    leaves, want = M.cached_tree(label, a, m)
    depth, n_nodes = M.shape(m, a)
    assert want.shape == (n_nodes, 4)
    nodes, root = _ctx(label).merkle_ragged(leaves, a)
    assert np.array_equal(nodes, want), (label, a, m)
    assert np.array_equal(root, want[-1])
    _, only_root = _ctx(label).merkle_ragged(leaves, a, want_nodes=False)
    assert np.array_equal(only_root, want[-1])
    # the device entry on an image whose non-leaf rows hold a non-zero pattern, with rows behind the root that must stay: a short parent
    # that reads past its level would absorb the pattern
    image = np.full((n_nodes + 4, 4), FILL, dtype=np.uint64)
    image[:m] = leaves
    d = _dev(image)
    _ctx(label).merkle_ragged_dev(d.data_ptr(), m, a, _stream())
    got = _host(d).reshape(n_nodes + 4, 4)
    assert np.array_equal(got[:n_nodes], want), (label, a, m)
    assert (got[n_nodes:] == FILL).all()


@pytest.mark.parametrize("label,a,m", POWERS)
def test_a_power_of_the_arity_is_the_ary_tree_byte_for_byte(label, a, m):
    f, cfg, cr = M.config(label)
    leaves, want = MA.cached_tree(label, a, m)
    nodes, root = _ctx(label).merkle_ragged(leaves, a)
    old_nodes, old_root = _ctx(label).merkle_ary(leaves, a)
    assert nodes.tobytes() == old_nodes.tobytes() and root.tobytes() == old_root.tobytes() and np.array_equal(nodes, want)
    image = np.full(want.shape, FILL, dtype=np.uint64)
    image[:m] = leaves
    d = _dev(image)
    _ctx(label).merkle_ragged_dev(d.data_ptr(), m, a, _stream())
    assert _host(d).tobytes() == old_nodes.tobytes()
    # openings, verdicts and an update through both families
    idx = MA.path_indices(m, a, 33, seed=1)
    paths = MA.open_paths(want, m, a, idx)
    depth = MA.shape(m, a)[0]
    d_nodes, d_idx = _dev(want), _dev(idx)
    outs = []
    for gather in (_ctx(label).merkle_ragged_paths_dev, _ctx(label).merkle_ary_paths_dev):
        d_paths = _dev(np.full(paths.shape, 0x77, dtype=np.uint64))
        gather(d_nodes.data_ptr(), m, a, d_idx.data_ptr(), len(idx), d_paths.data_ptr(), _stream())
        outs.append(_host(d_paths).tobytes())
    assert outs[0] == outs[1] == paths.tobytes()
    bad = paths.copy()
    bad[1::2, 0, 0, 0] ^= np.uint64(4)
    mine = leaves[idx.astype(np.int64)]
    v_new = _ctx(label).merkle_ragged_verify_paths(mine, idx, bad, depth, a, m, np.array(want[-1]))
    v_old = _ctx(label).merkle_ary_verify_paths(mine, idx, bad, depth, a, np.array(want[-1]))
    assert np.array_equal(v_new, v_old) and v_new.tolist() == [1 - i % 2 for i in range(len(idx))]
    if a == 2:
        two_nodes, two_root = _ctx(label).merkle_2to1(leaves)
        assert nodes.tobytes() == two_nodes.tobytes() and root.tobytes() == two_root.tobytes()
        assert np.array_equal(nodes, cr.merkle(leaves, threads=0))


@pytest.mark.parametrize("label,a,m,levels", TABLE)
def test_the_engine_report_names_the_engine_of_the_level(label, a, m, levels):
    """pmx_ctx_engine_info(PMX_OP_COMPRESS, W, arity) names the engine of a level of W parents: the quad engine for the t = 3 levels of
    at most 32768 parents, the window engine of t = 3 above"""
    for w in levels:
        want = b"HybridEngine<3,5" if label == "t3" and w > 32768 else ENGINE[label]
        info = _engine(label, w, a)
        assert info.engine.startswith(want), (label, w, info.engine)
        assert info.launches == 1


def test_the_fixture_of_the_big_integer_oracle():
    for name, v in golden("merkle_ragged_vectors.json").items():
        p, bits = FIELDS[v["field"]]
        f = S.BN254_FR if v["field"] == "bn254_fr" else S.BLS12_381_FR
        cfg = S.poseidon_config_from_lfsr(f, v["rate"], v["alpha"], v["full_rounds"], v["partial_rounds"])
        want = cref.elems_to_limbs([int(x, 16) for x in v["nodes"]], p)
        nodes, root = cfg.context().merkle_ragged(want[:v["n_leaves"]], v["arity"])
        assert np.array_equal(nodes, want) and np.array_equal(root, want[-1]), name


# ---- openings -----------------------------------------------------------------------------------------------------------------
def _gather_dev(label, a, m, nodes, idx):
    depth, _ = M.shape(m, a)
    k = len(idx)
    d_nodes, d_idx = _dev(nodes), _dev(idx)
    d_paths = _dev(np.full(max(k * depth * (a - 1) * 4, 4), 0x77, dtype=np.uint64))
    _ctx(label).merkle_ragged_paths_dev(d_nodes.data_ptr(), m, a, d_idx.data_ptr(), k, d_paths.data_ptr(), _stream())
    return _host(d_paths)[:k * depth * (a - 1) * 4].reshape(k, depth, a - 1, 4)


@pytest.mark.parametrize("k", PATH_COUNTS)
@pytest.mark.parametrize("label,a,m", PATH_TREES)
def test_host_and_device_openings_equal_the_oracle(label, a, m, k):
    leaves, nodes = M.cached_tree(label, a, m)
    depth, _ = M.shape(m, a)
    idx = M.path_indices(m, a, k, seed=k)
    if k >= 65:
        must = {0, m - 1} | {c * a ** level for level, c in M.short_children(m, a)}
        assert must <= set(int(i) for i in idx) and len(must) > 2
    want = M.open_paths(nodes, m, a, idx)
    host = np.full((k, depth, a - 1, 4), 0x33, dtype=np.uint64)
    _lib.check(_lib.lib().pmx_merkle_ragged_paths(_void(nodes), m, a, _void(idx), k, _void(host)))
    assert np.array_equal(host, want), "the host gather against the index arithmetic"
    got = _gather_dev(label, a, m, nodes, idx)
    assert np.array_equal(got, want), (label, a, m, k)
    # the opening of the last leaf: the siblings behind the level's end are exactly zero, in the oracle and so in both gathers
    w = M.widths(m, a)
    last, index = got[0], m - 1
    assert int(idx[0]) == m - 1
    absent = 0
    for level in range(depth):
        digit, base = index % a, index - index % a
        for s, c in enumerate(c for c in range(a) if c != digit):
            if base + c >= w[level]:
                assert not last[level, s].any()
                absent += 1
        index //= a
    assert absent > 0


def test_the_device_opening_of_an_index_that_names_no_leaf_is_zero():
    leaves, nodes = M.cached_tree("t9-bn254", 8, 513)
    idx = np.array([3, 513, 512, U64, 1 << 40, 519, 4095], dtype=np.uint64)      # (519: a slot of the short parent; 4095 < 8^4)
    got = _gather_dev("t9-bn254", 8, 513, nodes, idx)
    assert np.array_equal(got[[0, 2]], M.open_paths(nodes, 513, 8, idx[[0, 2]]))
    assert not got[[1, 3, 4, 5, 6]].any()


# ---- verification -------------------------------------------------------------------------------------------------------------
def _verify_both(label, a, m, mine, idx, paths, root):
    """the verdicts of the host entry and of the device entry (d_ok at an odd address)"""
    depth, k = M.shape(m, a)[0], len(idx)
    host = _ctx(label).merkle_ragged_verify_paths(mine, idx, paths, depth, a, m, root)
    d = [_dev(x) for x in (mine, idx, paths if paths.size else np.zeros(4, dtype=np.uint64), root)]
    d_ok = _dev(np.full(k + 1, 9, dtype=np.uint8))
    d_work = _dev(np.zeros(k * (a + 1) * 4, dtype=np.uint64))
    _ctx(label).merkle_ragged_verify_paths_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), depth, a, m, k, d[3].data_ptr(),
                                               d_ok.data_ptr() + 1, d_work.data_ptr(), _stream())
    ok = _host(d_ok, np.uint8)
    assert ok[0] == 9
    return host, ok[1:]


@pytest.mark.parametrize("k", PATH_COUNTS)
@pytest.mark.parametrize("label,a,m", PATH_TREES)
def test_every_opening_verifies_and_one_flipped_bit_does_not(label, a, m, k):
    f, cfg, cr = M.config(label)
    leaves, nodes = M.cached_tree(label, a, m)
    depth = M.shape(m, a)[0]
    idx = M.path_indices(m, a, k, seed=k)
    paths = M.open_paths(nodes, m, a, idx)
    mine = np.array(leaves[idx.astype(np.int64)])
    root = np.array(nodes[-1])
    for got in _verify_both(label, a, m, mine, idx, paths, root):
        assert got.tolist() == [1] * k, (label, a, m, k)
    # one bit flipped in path 0 - the opening of the last leaf, which has absent siblings: in the leaf, in a present sibling, in an
    # ABSENT (zero) sibling, and in the root (every path fails).  Expected verdicts are the oracle's climb over whole rows - what a
    # verifier computes - against the root.
    present = np.argwhere(paths[0].any(axis=2))
    absent = np.argwhere(~paths[0].any(axis=2))
    assert len(present) and len(absent)
    for what in ("leaf", "present", "absent", "root"):
        l2, p2, r2 = mine.copy(), paths.copy(), root.copy()
        if what == "leaf":
            l2[0, 1] ^= np.uint64(1) << np.uint64(17)
        elif what == "present":
            level, s = present[-1]
            p2[0, level, s, 2] ^= np.uint64(1)
        elif what == "absent":
            level, s = absent[0]
            p2[0, level, s, 0] ^= np.uint64(1)
        else:
            r2[3] ^= np.uint64(1) << np.uint64(5)
        top = MA.climb(cr, l2[:1], idx[:1], p2[:1], a)
        assert not np.array_equal(top[0], r2), what
        want = [0] * k if what == "root" else [0] + [1] * (k - 1)
        if what != "root" and k > 1:      # (another path of the batch may open the same leaf: it carries its own good copy)
            assert (paths[1:] == p2[1:]).all()
        for got in _verify_both(label, a, m, l2, idx, p2, r2):
            assert got.tolist() == want, (label, a, m, k, what)


def test_an_index_between_n_leaves_and_the_full_tree_is_rejected_even_with_a_path_that_climbs_to_the_root():
    """513 leaves at arity 8: leaf 512 is the only child of its parent.  `Leaf` 513 = a zero element with leaf 512 as its first sibling
    and zeros for the rest is a row of the same parent, so its path climbs to the root - the root does not bind n_leaves.  The verifier
    of the full tree of this depth accepts it; the one that is told n_leaves must not."""
    label, a, m = "t9-bn254", 8, 513
    f, cfg, cr = M.config(label)
    leaves, nodes = M.cached_tree(label, a, m)
    depth = M.shape(m, a)[0]
    real = M.open_paths(nodes, m, a, [512])
    forged = real.copy()
    forged[0, 0] = 0
    forged[0, 0, 0] = leaves[512]                                # sibling 0 of digit 1
    idx = np.array([513, 512, 519, 4095], dtype=np.uint64)
    paths = np.concatenate([forged, real, forged, real])
    paths[2, 0] = 0
    paths[2, 0, 0] = leaves[512]                                 # digit 7: sibling 0 is child 0
    mine = np.stack([np.zeros(4, dtype=np.uint64), leaves[512], np.zeros(4, dtype=np.uint64), leaves[512]])
    root = np.array(nodes[-1])
    top = MA.climb(cr, mine, idx, paths, a)
    assert (top[:3] == root).all() and not (top[3] == root).all(), "the oracle's whole-row climb reaches the root from slots 513 and 519"
    for got in _verify_both(label, a, m, mine, idx, paths, root):
        assert got.tolist() == [0, 1, 0, 0]
    assert _ctx(label).merkle_ary_verify_paths(mine, idx, paths, depth, a, root).tolist() == [1, 1, 1, 0], "why n_leaves is an argument"


def test_verification_at_depth_zero_compares_the_leaf_with_the_root():
    leaf, _ = M.cached_tree("t9-bn254", 8, 1)
    other = M.cached_tree("t9-bn254", 8, 513)[0][:1]
    leaves = np.concatenate([leaf, other, leaf])
    idx = np.array([0, 0, 1], dtype=np.uint64)
    for got in _verify_both("t9-bn254", 8, 1, leaves, idx, np.zeros((3, 0, 7, 4), dtype=np.uint64), np.array(leaf[0])):
        assert got.tolist() == [1, 0, 0]


def test_arity_two_climbs_through_the_shift_gather_of_the_2to1_verifier():
    """At arity 2 the verifiers of every family gather a level's rows with the 2-to-1 verifier's kernel (bit `level` of the index, not
    a division).  5 leaves (levels 5, 3, 2, 1: two of them with an absent sibling), BLS12-381 t = 3: every leaf's opening, an index
    equal to n_leaves and a path with a flipped word, host and device entry, against the oracle's climb.  Then 8 leaves through
    pmx_merkle_ary_verify_paths* at arity 2: the verdicts of pmx_merkle_verify_paths on the same bytes."""
    label, a, m = "t3", 2, 5
    f, cfg, cr = M.config(label)
    leaves, nodes = M.cached_tree(label, a, m)
    assert M.widths(m, a) == [5, 3, 2, 1]
    idx = np.array([0, 1, 2, 3, 4, m, 2], dtype=np.uint64)
    real = np.minimum(idx, np.uint64(m - 1)).astype(np.int64)          # the index that names no leaf carries the last leaf's opening
    paths, mine, root = M.open_paths(nodes, m, a, real), np.array(leaves[real]), np.array(nodes[-1])
    assert not paths[4, 0].any() and not paths[4, 1].any() and paths[4, 2].any(), "leaf 4 has no sibling on two levels"
    paths[6, 1, 0, 3] ^= np.uint64(1) << np.uint64(40)                  # a present sibling of leaf 2: node 0 of level 1
    top = M.climb(cr, mine, real, paths, a, m)
    want = [int(i < m and np.array_equal(t, root)) for i, t in zip(idx.tolist(), top)]
    assert want == [1, 1, 1, 1, 1, 0, 0]
    for got in _verify_both(label, a, m, mine, idx, paths, root):
        assert got.tolist() == want
    # a power of two: the arity-k verifier at arity 2 and the 2-to-1 verifier read the same bytes ([k][depth][1][4] is [k][depth][4])
    m = 8
    leaves, nodes = M.cached_tree(label, a, m)
    idx = np.array([0, 1, 2, 3, 4, 5, 6, 7, m, 2], dtype=np.uint64)
    real = np.minimum(idx, np.uint64(m - 1)).astype(np.int64)
    paths, mine, root = M.open_paths(nodes, m, a, real), np.array(leaves[real]), np.array(nodes[-1])
    paths[9, 1, 0, 3] ^= np.uint64(1) << np.uint64(40)
    k, ctx = len(idx), _ctx(label)
    want = S.verify_paths(cfg, mine, idx, paths.reshape(k, 3, 4), root).astype(np.uint8).tolist()
    assert want == [1] * 8 + [0, 0]
    assert want == [int(i < m and np.array_equal(t, root)) for i, t in zip(idx.tolist(), M.climb(cr, mine, real, paths, a, m))]
    assert ctx.merkle_ary_verify_paths(mine, idx, paths, 3, a, root).tolist() == want
    d = [_dev(x) for x in (mine, idx, paths, root)]
    d_ok, d_work = _dev(np.full(k + 1, 9, dtype=np.uint8)), _dev(np.zeros(k * (a + 1) * 4, dtype=np.uint64))
    ctx.merkle_ary_verify_paths_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 3, a, k, d[3].data_ptr(), d_ok.data_ptr() + 1,
                                    d_work.data_ptr(), _stream())
    assert _host(d_ok, np.uint8).tolist() == [9] + want


# ---- updates ------------------------------------------------------------------------------------------------------------------
def _update_case(label, a, m, k, wild):
    """(indices, new leaves, old tree with marked rows, expected array).  Distinct indices that include the last leaf - under the only
    child of a short parent where the tree has one.  Rows of the levels that only the gathers read which are neither an ancestor of an
    update nor a sibling of one carry a mark: they must come back as they went in."""
    f, cfg, cr = M.config(label)
    leaves, old = M.cached_tree(label, a, m)
    w = M.widths(m, a)
    picks = list(dict.fromkeys([m - 1, 0] + [int(x) for x in np.random.default_rng(k).permutation(m)]))[:k]
    idx = np.array(picks, dtype=np.uint64)
    new = synth.random_elements(f, k, seed=900 + k)
    if wild and k >= 3:
        idx[1], idx[2] = m, U64
        if k > 3:
            idx[3] = m + 6
    after = np.array(leaves, dtype=np.uint64)
    live = [(int(j), i) for i, j in enumerate(idx) if int(j) < m]
    for j, i in live:
        after[j] = new[i]
    want = M.tree(cr, after, a)
    # the level whose nodes the first whole-level launch reads: below it only gathers read
    switch = next((l for l in range(len(w) - 1) if k >= w[l + 1]), len(w) - 1)
    start = np.array(old, dtype=np.uint64)
    first, marked = 0, 0
    for level in range(len(w) - 1):
        if 1 <= level < switch:
            touched = set()
            for j, _ in live:
                node = j // a ** level
                touched |= set(range(node - node % a, node - node % a + a))
            for c in range(w[level]):
                if c not in touched:
                    start[first + c, 0] ^= np.uint64(0xFFFF)
                    want[first + c] = start[first + c]
                    marked += 1
        first += w[level]
    return idx, new, start, want, marked


@pytest.mark.parametrize("wild", [False, True])
@pytest.mark.parametrize("label,a,m,counts", UPDATE_TREES)
def test_an_update_gives_the_rebuilt_tree_and_leaves_other_rows_alone(label, a, m, counts, wild):
    w = M.widths(m, a)
    assert counts[-1] >= w[1], "the last count runs whole levels from the first level on"
    any_marked = 0
    for k in counts:
        idx, new, start, want, marked = _update_case(label, a, m, k, wild)
        any_marked += marked
        d_nodes, d_idx, d_new = _dev(np.concatenate([start, np.full((2, 4), FILL, dtype=np.uint64)])), _dev(idx), _dev(new)
        d_work = _dev(np.zeros(k * (a + 1) * 4, dtype=np.uint64))
        _ctx(label).merkle_ragged_update_dev(d_nodes.data_ptr(), m, a, d_idx.data_ptr(), d_new.data_ptr(), k, d_work.data_ptr(), _stream())
        got = _host(d_nodes).reshape(-1, 4)
        assert np.array_equal(got[:-2], want), (label, a, m, k, wild)
        assert (got[-2:] == FILL).all()
    assert any_marked > 0, "some count keeps marked rows below the whole-level switch"


def test_an_update_of_indices_that_name_no_leaf_writes_nothing():
    label, a, m = "t9-bn254", 8, 513
    leaves, nodes = M.cached_tree(label, a, m)
    idx = np.array([513, 519, 520, U64, 4095, 1 << 33], dtype=np.uint64)
    new = synth.random_elements(M.config(label)[0], len(idx), seed=5)
    d_nodes, d_idx, d_new = _dev(nodes), _dev(idx), _dev(new)
    d_work = _dev(np.zeros(len(idx) * (a + 1) * 4, dtype=np.uint64))
    _ctx(label).merkle_ragged_update_dev(d_nodes.data_ptr(), m, a, d_idx.data_ptr(), d_new.data_ptr(), len(idx), d_work.data_ptr(), _stream())
    assert np.array_equal(_host(d_nodes).reshape(-1, 4), nodes)


# ---- refusals: the status, and nothing written ---------------------------------------------------------------------------------
def test_every_refusal_returns_its_status_and_writes_nothing():
    label, a, m = "t9-bn254", 8, 100
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
    v = _void

    def calls(h, arity, n_leaves=m, dep=depth, nodes_ptr=None):
        dn = p(d_nodes) if nodes_ptr is None else nodes_ptr
        return [
            ("ragged", lambda: L.pmx_merkle_ragged(h, v(leaves), n_leaves, arity, v(h_nodes), v(h_root))),
            ("ragged_dev", lambda: L.pmx_merkle_ragged_dev(h, dn, n_leaves, arity, s)),
            ("paths_dev", lambda: L.pmx_merkle_ragged_paths_dev(h, dn, n_leaves, arity, p(d_idx), k, p(d_out), s)),
            ("verify", lambda: L.pmx_merkle_ragged_verify_paths(h, v(leaves), v(idx), v(paths), dep, arity, n_leaves, k, v(h_root), v(h_ok))),
            ("verify_dev", lambda: L.pmx_merkle_ragged_verify_paths_dev(h, p(d_leaves), p(d_idx), p(d_paths), dep, arity, n_leaves, k, p(d_root),
                                                                        p(d_ok), p(d_work), s)),
            ("update_dev", lambda: L.pmx_merkle_ragged_update_dev(h, dn, n_leaves, arity, p(d_idx), p(d_leaves), k, p(d_work), s)),
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
        expect(_lib.PMX_ERR_ARG, calls(ctx._h, arity))
    expect(_lib.PMX_ERR_ARG, calls(ctx._h, a, n_leaves=0))       # no leaves
    expect(_lib.PMX_ERR_ARG, calls(ctx._h, a, n_leaves=1 << 60), b"overflow")
    # a depth that is not the depth of (n_leaves, arity)
    for dep in (depth - 1, depth + 1, 0):
        expect(_lib.PMX_ERR_ARG, calls(ctx._h, a, dep=dep), b"depth", only=("verify", "verify_dev"))
    expect(_lib.PMX_ERR_ARG, calls(None, a), b"null pointer")
    assert L.pmx_merkle_ragged(ctx._h, None, m, a, v(h_nodes), v(h_root)) == _lib.PMX_ERR_ARG
    assert L.pmx_merkle_ragged_dev(ctx._h, None, m, a, s) == _lib.PMX_ERR_ARG
    for hole in range(3):
        args = [p(d_nodes), p(d_idx), p(d_out)]
        args[hole] = None
        assert L.pmx_merkle_ragged_paths_dev(ctx._h, args[0], m, a, args[1], k, args[2], s) == _lib.PMX_ERR_ARG, hole
    for hole in range(6):
        args = [p(d_leaves), p(d_idx), p(d_paths), p(d_root), p(d_ok), p(d_work)]
        args[hole] = None
        assert L.pmx_merkle_ragged_verify_paths_dev(ctx._h, args[0], args[1], args[2], depth, a, m, k, args[3], args[4], args[5], s) == _lib.PMX_ERR_ARG, hole
    for hole in range(5):
        args = [v(leaves), v(idx), v(paths), v(h_root), v(h_ok)]
        args[hole] = None
        assert L.pmx_merkle_ragged_verify_paths(ctx._h, args[0], args[1], args[2], depth, a, m, k, args[3], args[4]) == _lib.PMX_ERR_ARG, hole
    for hole in range(4):
        args = [p(d_nodes), p(d_idx), p(d_leaves), p(d_work)]
        args[hole] = None
        assert L.pmx_merkle_ragged_update_dev(ctx._h, args[0], m, a, args[1], args[2], k, args[3], s) == _lib.PMX_ERR_ARG, hole
    untouched()
    # an element array that is not 16-byte aligned
    expect(_lib.PMX_ERR_ARG, calls(ctx._h, a, nodes_ptr=p(d_nodes) + 8), b"16-byte aligned", only=("ragged_dev", "paths_dev", "update_dev"))
    # arity beyond the rate: a configuration error that points at the hash driver (rate 3 here)
    for name, call in calls(_ctx("t4")._h, 4, dep=M.shape(m, 4)[0]):
        assert call() == _lib.PMX_ERR_CONFIG, (name, L.pmx_last_error())
        assert b"pmx_hash_batch_dev" in L.pmx_last_error() and b"rate" in L.pmx_last_error()
        untouched()
    # k = 0 asks for nothing
    assert L.pmx_merkle_ragged_update_dev(ctx._h, None, m, a, None, None, 0, None, s) == _lib.PMX_OK
    assert L.pmx_merkle_ragged_paths_dev(ctx._h, None, m, a, None, 0, None, s) == _lib.PMX_OK
    untouched()
    got, _ = ctx.merkle_ragged(leaves, a)
    assert np.array_equal(got, nodes)


# ---- the Python tree ------------------------------------------------------------------------------------------------------------
def test_the_python_tree_builds_opens_updates_and_verifies():
    label, a, m = "t9-bn254", 8, 1000
    f, cfg, cr = M.config(label)
    leaves, nodes = M.cached_tree(label, a, m)
    tree = S.MerkleTree(cfg, leaves, arity=a)
    assert tree.ragged and tree.depth == 4 and tree.level_widths() == [1000, 125, 16, 2, 1]
    assert np.array_equal(tree.nodes, nodes) and np.array_equal(tree.root, nodes[-1])
    assert tree.level_offset(1) == 1000 and tree.level_offset(3) == 1141 and tree.level_offset(tree.depth) == nodes.shape[0] - 1
    idx = M.path_indices(m, a, 20, seed=5)
    want = M.open_paths(nodes, m, a, idx)
    paths = tree.paths(idx)
    assert np.array_equal(paths, want) and np.array_equal(tree.paths_dev(idx), want)
    assert np.array_equal(tree.path(999), want[0]) and not want[0, 1, 5:].any()      # (node 124 of level 1 has no sibling behind it)
    mine = leaves[idx.astype(np.int64)]
    assert S.verify_paths(cfg, mine, idx, paths, tree.root, arity=a, n_leaves=m).all()
    bad = paths.copy()
    bad[3, 1, 2, 0] ^= np.uint64(1)
    ok = S.verify_paths(cfg, mine, idx, bad, tree.root, arity=a, n_leaves=m)
    assert not ok[3] and ok.sum() == 19
    with pytest.raises(_lib.PmxError, match="out of range"):
        tree.paths([1000])
    # update: the last duplicate wins, a bad index changes nothing
    new = synth.random_elements(f, 4, seed=77)
    with pytest.raises(_lib.PmxError, match="out of range"):
        tree.update([5, 1000], new[:2])
    assert np.array_equal(tree.nodes, nodes)
    tree.update([999, 5, 999, 124], new)
    after = np.array(leaves, dtype=np.uint64)
    after[5], after[999], after[124] = new[1], new[2], new[3]
    rebuilt = M.tree(cr, after, a)
    assert np.array_equal(tree.nodes, rebuilt) and np.array_equal(tree.root, rebuilt[-1])
    # a power of the arity is the tree it always was; arity 2 takes any count too
    l2, n2 = M.cached_tree("t3", 2, 100)
    t2 = S.MerkleTree(M.config("t3")[1], l2)
    assert t2.ragged and t2.arity == 2 and np.array_equal(t2.nodes, n2) and t2.paths([99]).shape == (1, 7, 4)
    assert S.verify_paths(M.config("t3")[1], l2[[99]], [99], t2.paths([99]), t2.root, n_leaves=100).all()
    assert not S.MerkleTree(cfg, MA.cached_tree(label, 8, 512)[0], arity=8).ragged
