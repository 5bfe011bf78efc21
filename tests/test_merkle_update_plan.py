"""Leaf updates of a Merkle tree (include/poseidon_mi355x.h: pmx_merkle_ary_update, pmx_merkle_ary_update_dev) on the CPU.

- The host plan (sponge_amd/csrc/pmx_merkle_plan.hpp) compiled for the host behind tests/merkle_plan/merkle_plan_c.cpp: the device's share
  of pmx_merkle_ary_update - compress the rows of a level, scatter the digests to their slots of the next level's rows - is replayed here
  with the C port's batch hash, and the node array must come out as the C port's full rebuild over the updated leaf row.
- The index arithmetic of node_scatter_kernel and node_children_kernel (pmx_tree_moves.hip) and the level loop of pmx_merkle_ary_update_dev,
  restated lane by lane, against the same rebuild.
- The argument checks of both entries that fire before a device is needed.
- tests/merkle_plan/sanitize_main.cpp, a program of its own, under ASan + UBSan.
Expected values never come from the product: merkle_ary_oracle.tree over the leaves with the updates applied."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from sponge_amd import _lib, synth

import merkle_ary_oracle as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "merkle_plan")
CSRC = os.path.join(ROOT, "sponge_amd", "csrc")
LABEL = {2: "t3", 3: "t4", 8: "t9-bn254", 15: "lds-t16"}
U64 = (1 << 64) - 1
_sz, _p = ctypes.c_size_t, ctypes.c_void_p


@pytest.fixture(scope="module")
def mp(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("merkle_plan") / "libmerkle_plan.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-DPMX_HOSTCHECK", "-I", CSRC,
                           os.path.join(HERE, "merkle_plan_c.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.mp_build.restype, lib.mp_build.argtypes = _p, [_p, _sz, ctypes.c_uint32, _p, _p, _sz]
    lib.mp_free.restype, lib.mp_free.argtypes = None, [_p]
    lib.mp_first_bad.restype, lib.mp_first_bad.argtypes = _sz, [_p, _sz, _sz]
    for name in ("mp_depth", "mp_n_rows", "mp_upload_words"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _sz, [_p]
    for name in ("mp_level_size", "mp_level_first", "mp_row_first"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _sz, [_p, _sz]
    lib.mp_level.restype, lib.mp_level.argtypes = _p, [_p, _sz]
    lib.mp_rows.restype, lib.mp_rows.argtypes = _p, [_p]
    lib.mp_slots.restype, lib.mp_slots.argtypes = _p, [_p]
    lib.mp_apply.restype, lib.mp_apply.argtypes = None, [_p, _p, _p, _p]
    return lib


def _view(addr, words):
    if words == 0:
        return np.zeros(0, dtype=np.uint64)
    return np.ctypeslib.as_array((ctypes.c_uint64 * words).from_address(addr))


def updated_leaves(leaves, idx, new):
    """the leaf row after the updates in call order (duplicates: the last one wins)"""
    out = np.array(leaves, dtype=np.uint64)
    for i, j in enumerate(int(x) for x in idx):
        out[j] = new[i]
    return out


def distinct_ancestors(idx, a, depth):
    """the (level, node) pairs above the updated leaves, counted one leaf at a time"""
    seen = set()
    for j in (int(x) for x in idx):
        for level in range(1, depth + 1):
            seen.add((level, j // a ** level))
    return seen


def index_sets(m, a, seed):
    rng = np.random.default_rng(seed)
    sets = {
        "none": [],
        "first": [0],
        "last": [m - 1],
        "ends": [0, m - 1],
        "duplicates": [0, m - 1, 0, m // 2, m - 1, 0],
        "one parent": [m - 1 - c for c in range(min(a, m))],
        "random": list(rng.integers(0, m, 40)),
        "all": list(rng.permutation(m)),
    }
    if m <= 4096:
        sets["all twice"] = list(rng.permutation(m)) + list(rng.permutation(m))
    for k in (2, 3, a + 1, m // a, m // a + 1, m - 1):
        if 0 < k <= m:
            sets["%d distinct" % k] = list(rng.choice(m, k, replace=False))
    return sets


@pytest.mark.parametrize("depth", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("a", [2, 3, 8, 15])
def test_replayed_plan_equals_the_full_rebuild(mp, a, depth):
    f, cfg, cr = M.config(LABEL[a])
    m = a ** depth
    leaves, nodes = M.cached_tree(LABEL[a], a, m)
    first = [sum(m // a ** j for j in range(l)) for l in range(depth + 1)]
    for name, raw in index_sets(m, a, seed=100 * a + depth).items():
        idx = np.array(raw, dtype=np.uint64)
        k = len(idx)
        new = synth.random_elements(f, max(k, 1), seed=7000 + 10 * a + depth + k)[:k]
        want = M.tree(cr, updated_leaves(leaves, idx, new), a)
        assert mp.mp_first_bad(idx.ctypes.data, k, m) == k
        old = nodes.copy()
        h = mp.mp_build(old.ctypes.data, m, a, idx.ctypes.data, new.ctypes.data, k)
        try:
            assert np.array_equal(old, nodes), "the plan reads the node array, it writes nothing"
            assert mp.mp_depth(h) == depth
            assert [mp.mp_level_first(h, l) for l in range(depth + 1)] == first
            levels = [_view(mp.mp_level(h, l), mp.mp_level_size(h, l)).copy() for l in range(depth + 1)]
            # S_l: sorted, distinct, exactly the nodes above the updates; the permutations: each distinct ancestor once
            anc = distinct_ancestors(idx, a, depth)
            assert [int(x) for x in levels[0]] == sorted(set(int(x) for x in idx))
            for l in range(1, depth + 1):
                assert [int(x) for x in levels[l]] == sorted(q for lv, q in anc if lv == l), (name, l)
            n_rows = mp.mp_n_rows(h)
            assert n_rows == sum(len(s) for s in levels[1:]) == len(anc), name
            assert mp.mp_upload_words(h) == n_rows * a * 4 + n_rows
            rows = _view(mp.mp_rows(h), n_rows * a * 4).reshape(n_rows, a, 4)
            slots = _view(mp.mp_slots(h), n_rows)
            digests = np.zeros((n_rows, 4), dtype=np.uint64)
            for l in range(1, depth + 1):          # the device's share
                r, count = mp.mp_row_first(h, l), len(levels[l])
                assert mp.mp_row_first(h, l + 1) == r + count
                if not count:
                    continue
                digests[r:r + count] = cr.hash_batch(rows[r:r + count], a, 1, threads=0).reshape(count, 4)
                if l < depth:
                    nxt, width = mp.mp_row_first(h, l + 1), len(levels[l + 1]) * a
                    flat = rows.reshape(-1, 4)
                    rank = {int(q): at for at, q in enumerate(levels[l + 1])}
                    for j in range(count):
                        s = int(slots[r + j])
                        assert s < width and s == rank[int(levels[l][j]) // a] * a + int(levels[l][j]) % a
                        flat[nxt * a + s] = digests[r + j]
            got = nodes.copy()
            mp.mp_apply(h, new.ctypes.data, digests.ctypes.data, got.ctypes.data)
        finally:
            mp.mp_free(h)
        assert np.array_equal(got, want), (a, depth, name)
        # nothing but leaves and ancestors was written
        touched = {int(x) for x in idx} | {first[l] + q for l, q in anc}
        rest = np.array(sorted(set(range(len(nodes))) - touched), dtype=np.int64)
        assert np.array_equal(got[rest], nodes[rest])


def test_first_bad_index(mp):
    for bad, at in (([81], 0), ([5, 80, 81], 2), ([1 << 63, 3], 0), ([5, U64], 1), ([0, 80], 2), ([], 0)):
        idx = np.array(bad, dtype=np.uint64)
        assert mp.mp_first_bad(idx.ctypes.data, len(bad), 81) == at


# ---- the device entry, lane by lane -----------------------------------------------------------------------------------------------
def scatter_lanes(src, indices, pow_, limit, base, dst, k):
    """node_scatter_kernel: src [k*2] and dst [..] in 16-byte halves (rows of 2 words)"""
    for gid in range((k * 2 + 255) // 256 * 256):
        i = gid >> 1
        if i >= k:
            continue
        idx = int(indices[i])
        if idx >= limit:
            continue
        at = (base + idx // pow_) * 2 + (gid & 1)
        assert 0 <= at < len(dst), "a store outside the array"
        dst[at] = src[gid]


def children_lanes(nodes, indices, pow_, n_leaves, first, a, rows, k):
    """node_children_kernel"""
    per = 2 * a
    for gid in range((k * per + 255) // 256 * 256):
        i = gid // per
        if i >= k:
            continue
        idx = int(indices[i])
        p = idx // pow_ if idx < n_leaves else 0
        at = (first + p * a) * 2 + (gid - i * per)
        assert 0 <= at < len(nodes), "a load outside the array"
        rows[gid] = nodes[at]


def update_dev_emulated(cr, nodes, m, a, indices, new, launches):
    """the level loop of pmx_merkle_ary_update_dev over halves [n][2]; launches collects (kind, units)"""
    k, depth = len(indices), M.shape(m, a)[0]
    halves = nodes.reshape(-1, 2)
    cur = np.zeros((k * 2, 2), dtype=np.uint64)
    rows = np.zeros((k * a * 2, 2), dtype=np.uint64)
    scatter_lanes(new.reshape(-1, 2), indices, 1, m, 0, halves, k)
    first, width, pow_ = 0, m, a
    for l in range(depth):
        parents = width // a
        if k >= parents:
            while width > 1:
                lv = halves[first * 2:(first + width) * 2].reshape(width // a, a, 4)
                halves[(first + width) * 2:(first + width + width // a) * 2] = cr.hash_batch(lv, a, 1, threads=0).reshape(-1, 2)
                launches.append(("level", width // a))
                first, width = first + width, width // a
            break
        children_lanes(halves, indices, pow_, m, first, a, rows, k)
        cur[:] = cr.hash_batch(rows.reshape(k, a, 4), a, 1, threads=0).reshape(-1, 2)
        launches.append(("gather", k))
        scatter_lanes(cur, indices, pow_, m, first + width, halves, k)
        first, width, pow_ = first + width, parents, pow_ * a


DEV_CASES = [("t3", 2, 64), ("t4", 3, 81), ("t9-bn254", 8, 512), ("t9-bn254", 5, 125), ("lds-t16", 15, 225), ("t4", 3, 1)]


@pytest.mark.parametrize("label,a,m", DEV_CASES)
def test_kernel_index_arithmetic_equals_the_full_rebuild(label, a, m):
    f, cfg, cr = M.config(label)
    leaves, nodes = M.cached_tree(label, a, m)
    W = max(m // a, 1)
    rng = np.random.default_rng(m + a)
    for k in sorted({1, 2, 5, W - 1, W, W + 1, m} - {0}):
        k_real = min(k, m)
        idx = list(rng.choice(m, k_real, replace=False))
        idx[0] = m - 1
        if k_real > 1:
            idx[1] = 0 if idx[0] != 0 else 1
            idx = list(dict.fromkeys(int(x) for x in idx))
            k_real = len(idx)
        new = synth.random_elements(f, k_real + 3, seed=31 * m + k)
        want = M.tree(cr, updated_leaves(leaves, idx, new), a)
        # in range only; then with indices that name no leaf mixed in (ignored), and an equal-index equal-leaf duplicate
        for extra in ([], [m, U64, idx[0]]):
            all_idx = np.array(idx + extra, dtype=np.uint64)
            all_new = np.concatenate([new[:k_real], new[k_real:k_real + 2], new[0:1]])[:len(all_idx)]
            got, launches = nodes.copy(), []
            update_dev_emulated(cr, got, m, a, all_idx, all_new, launches)
            assert np.array_equal(got, want), (label, a, m, k, extra)
            kk = len(all_idx)
            gathered = [n for kind, n in launches if kind == "gather"]
            whole = [n for kind, n in launches if kind == "level"]
            assert all(n == kk for n in gathered) and all(kk >= n for n in whole[:1])
            assert sum(gathered) + sum(whole) <= min(kk * M.shape(m, a)[0], (m - 1) // (a - 1)), "never more permutations than a rebuild"
            assert len(gathered) + len(whole) == M.shape(m, a)[0]


def test_an_out_of_range_index_alone_changes_nothing():
    f, cfg, cr = M.config("t4")
    leaves, nodes = M.cached_tree("t4", 3, 81)
    got = nodes.copy()
    # (a consistent tree: the whole level at the top rewrites the root with its own value)
    new = synth.random_elements(f, 2, seed=5)
    update_dev_emulated(cr, got, 81, 3, np.array([81, U64], dtype=np.uint64), new, [])
    assert np.array_equal(got, nodes)


# ---- argument checks that need no device -----------------------------------------------------------------------------------------
def test_update_entries_refuse_bad_arguments_before_a_device_is_needed():
    L = _lib.lib()
    buf = np.zeros(4096, dtype=np.uint64)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16       # a 16-byte aligned address inside buf
    fake = ctypes.c_void_p(base)                            # a context handle that is never dereferenced: the checks come first
    nodes, idx, new, work = _p(base + 1024), _p(base + 8192), _p(base + 9216), _p(base + 16384)
    dev, host = L.pmx_merkle_ary_update_dev, L.pmx_merkle_ary_update
    # arity below 2, a leaf count that is no power of the arity
    for n, a in ((81, 1), (81, 0), (80, 3), (0, 3), (54, 3), (81, 2), (1 << 63, 3)):
        assert dev(fake, nodes, n, a, idx, new, 1, work, None) == _lib.PMX_ERR_ARG, (n, a)
        assert host(fake, nodes, n, a, idx, new, 1, None) == _lib.PMX_ERR_ARG, (n, a)
    assert b"power of the arity" in L.pmx_last_error() or b"overflow" in L.pmx_last_error()
    # null pointers
    assert dev(None, nodes, 81, 3, idx, new, 1, work, None) == _lib.PMX_ERR_ARG
    for args in ((None, 81, 3, idx, new, 1, work), (nodes, 81, 3, None, new, 1, work), (nodes, 81, 3, idx, None, 1, work),
                 (nodes, 81, 3, idx, new, 1, None)):
        assert dev(fake, *args, None) == _lib.PMX_ERR_ARG, args
        assert b"null" in L.pmx_last_error()
    assert host(None, nodes, 81, 3, idx, new, 1, None) == _lib.PMX_ERR_ARG
    for args in ((None, 81, 3, idx, new, 1), (nodes, 81, 3, None, new, 1), (nodes, 81, 3, idx, None, 1)):
        assert host(fake, *args, None) == _lib.PMX_ERR_ARG, args
        assert b"null" in L.pmx_last_error()
    # misaligned element arrays and indices
    for args in ((_p(base + 1024 + 8), idx, new, work), (nodes, idx, _p(base + 9216 + 8), work), (nodes, idx, new, _p(base + 16384 + 8)),
                 (nodes, _p(base + 8192 + 4), new, work)):
        assert dev(fake, args[0], 81, 3, args[1], args[2], 1, args[3], None) == _lib.PMX_ERR_ARG, args
        assert b"aligned" in L.pmx_last_error()
    # host: an index that names no leaf is refused by name, before anything is modified
    tree = np.full((121, 4), 7, dtype=np.uint64)
    fresh = np.full((3, 4), 9, dtype=np.uint64)
    root = np.full(4, 5, dtype=np.uint64)
    for bad in ([81], [5, 80, 81], [1 << 63, 2], [5, U64, 6]):
        ix = np.array(bad, dtype=np.uint64)
        assert host(fake, _p(tree.ctypes.data), 81, 3, _p(ix.ctypes.data), _p(fresh.ctypes.data), len(bad), _p(root.ctypes.data)) == _lib.PMX_ERR_ARG
        assert b"out of range" in L.pmx_last_error() and str(max(bad)).encode() in L.pmx_last_error()
        assert (tree == 7).all() and (root == 5).all(), "a refused update writes nothing"


def test_the_python_surface_has_the_update():
    import sponge_amd as S
    from sponge_amd.poseidon import Context
    assert callable(S.MerkleTree.update) and callable(Context.merkle_ary_update) and callable(Context.merkle_ary_update_dev)
    assert "pmx_merkle_ary_update" in _lib.SIGNATURES and "pmx_merkle_ary_update_dev" in _lib.SIGNATURES


# ---- the plan under the sanitizers: a program of its own, nothing sanitized is loaded into this process ----------------------------
def test_plan_header_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "merkle_plan_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-DPMX_HOSTCHECK", "-I", CSRC, os.path.join(HERE, "sanitize_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and "sanitized ok" in out.stdout, out.stdout + out.stderr
