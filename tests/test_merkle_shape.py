"""The layout of a Merkle tree (sponge_amd/csrc/pmx_merkle_shape.hpp), compiled for the host behind tests/merkle_shape/merkle_shape_c.cpp,
against a few lines of Python with unbounded integers: depth, node count and every level's {first, width} for every leaf count 1 .. 2000
at every arity 2 .. 16, in both modes (exact accepts exactly the powers of the arity); the level at which a leaf update switches to whole
levels; and both sides of every bound at which a size stops fitting.  tests/merkle_shape/sanitize_main.cpp, a program of its own, walks the
same ground under ASan + UBSan.  Expected values never come from the header."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "merkle_shape")
CSRC = os.path.join(ROOT, "sponge_amd", "csrc")
SIZE_MAX = (1 << 64) - 1
OK, ARITY, NO_LEAVES, NOT_POWER, TREE_OVERFLOW, NO_TREES, FOREST_OVERFLOW, POW_OVERFLOW = range(8)
ARITIES = range(2, 17)
_sz, _u32, _p = ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p


@pytest.fixture(scope="module")
def ms(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("merkle_shape") / "libmerkle_shape.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", CSRC, os.path.join(HERE, "merkle_shape_c.cpp"),
                           "-o", out])
    lib = ctypes.CDLL(out)
    lib.ms_shape.restype, lib.ms_shape.argtypes = ctypes.c_int, [_sz, _u32, ctypes.c_int, _p, _p]
    lib.ms_forest.restype, lib.ms_forest.argtypes = ctypes.c_int, [_sz, _sz, _u32, ctypes.c_int, _p, _p]
    lib.ms_leaves_of_depth.restype, lib.ms_leaves_of_depth.argtypes = ctypes.c_int, [_u32, _sz, _p]
    lib.ms_switch_level.restype, lib.ms_switch_level.argtypes = _sz, [_sz, _u32, _sz]
    lib.ms_walk.restype, lib.ms_walk.argtypes = _sz, [_sz, _u32, _p, _p, _sz]
    return lib


def levels(n, a):
    """[(first, width)] from the leaves to the root: level l + 1 has ceil(width_l / a) nodes"""
    out, first = [], 0
    while True:
        out.append((first, n))
        if n == 1:
            return out
        first, n = first + n, -(-n // a)


def is_power(n, a):
    while n > 1 and n % a == 0:
        n //= a
    return n == 1


def shape(ms, n, a, exact):
    """(code, depth, n_nodes); a refused shape must write nothing"""
    depth, nodes = _sz(12345), _sz(12345)
    rc = ms.ms_shape(n, a, int(exact), ctypes.byref(depth), ctypes.byref(nodes))
    if rc != OK:
        assert (depth.value, nodes.value) == (12345, 12345)
    return rc, depth.value, nodes.value


def want_shape(n, a, exact):
    """the rule of the header, in unbounded integers: level by level, a width that no longer fits is refused before it is tested for dividing"""
    if a < 2:
        return ARITY
    if n == 0:
        return NO_LEAVES
    nodes = 0
    for first, width in levels(n, a):
        if width > SIZE_MAX // 32 - nodes:
            return TREE_OVERFLOW
        nodes += width
        if width > 1 and exact and width % a:
            return NOT_POWER
    return OK


def forest(ms, n_trees, lpt, a, pair_bound):
    tl, tn = _sz(777), _sz(777)
    rc = ms.ms_forest(n_trees, lpt, a, int(pair_bound), ctypes.byref(tl), ctypes.byref(tn))
    if rc != OK:
        assert (tl.value, tn.value) == (777, 777)
    return rc, tl.value, tn.value


def leaves_of_depth(ms, a, depth):
    out = ctypes.c_uint64(999)
    rc = ms.ms_leaves_of_depth(a, depth, ctypes.byref(out))
    if rc != OK:
        assert out.value == 999
    return rc, out.value


@pytest.mark.parametrize("a", ARITIES)
def test_every_leaf_count_up_to_2000(ms, a):
    first, width = (_sz * 16)(), (_sz * 16)()
    powers = 0
    for n in range(1, 2001):
        lv = levels(n, a)
        depth, nodes = len(lv) - 1, sum(w for _, w in lv)
        assert shape(ms, n, a, False) == (OK, depth, nodes), n
        if is_power(n, a):
            powers += 1
            assert shape(ms, n, a, True) == (OK, depth, nodes), n
        else:
            assert shape(ms, n, a, True)[0] == NOT_POWER, n
        assert ms.ms_walk(n, a, first, width, 16) == len(lv)
        assert [(first[l], width[l]) for l in range(len(lv))] == lv, n
        # the update's switch: the first level whose parents are no more than k, the depth if there is none
        for l in range(depth):
            parents = lv[l + 1][1]
            for k in {1, 2, parents - 1, parents, parents + 1} - {0}:
                want = next((j for j in range(depth) if k >= lv[j + 1][1]), depth)
                assert ms.ms_switch_level(n, a, k) == want, (n, k)
        assert ms.ms_switch_level(n, a, 1) == (depth - 1 if depth else 0)      # one update: every level but the root's is a gather
    assert powers == len([d for d in range(64) if a ** d <= 2000])


def test_arity_and_leaf_count_are_checked_first(ms):
    for a in (0, 1):
        for n in (0, 1, 8, SIZE_MAX):
            assert shape(ms, n, a, False)[0] == shape(ms, n, a, True)[0] == ARITY
        assert forest(ms, 0, 0, a, False)[0] == ARITY and leaves_of_depth(ms, a, 3)[0] == ARITY
    for a in (2, 3, 16, 0xffffffff):
        assert shape(ms, 0, a, False)[0] == shape(ms, 0, a, True)[0] == NO_LEAVES
        assert shape(ms, 1, a, True) == shape(ms, 1, a, False) == (OK, 0, 1)


@pytest.mark.parametrize("a", ARITIES)
def test_tree_bytes_overflow_on_both_sides(ms, a):
    """n_nodes * 32 must fit a size_t: refused when width > SIZE_MAX / 32 - nodes at any level"""
    # every power of the arity in a size_t; the largest one's node count still fits 64 bits, its bytes do not
    n, seen = 1, set()
    while n <= SIZE_MAX:
        lv = levels(n, a)
        fits = sum(w for _, w in lv) * 32 <= SIZE_MAX
        want = (OK, len(lv) - 1, sum(w for _, w in lv)) if fits else (TREE_OVERFLOW, 12345, 12345)
        assert shape(ms, n, a, True) == shape(ms, n, a, False) == want, n
        seen.add(fits)
        last, n = n, n * a
    assert seen == {True, False} and sum(w for _, w in levels(last, a)) <= SIZE_MAX < sum(w for _, w in levels(last, a)) * 32
    # the leaves alone fill the bound: SIZE_MAX / 32 of them and one more, then the largest count that fits, by bisection
    for n in (SIZE_MAX // 32, SIZE_MAX // 32 + 1, SIZE_MAX):
        assert shape(ms, n, a, False)[0] == TREE_OVERFLOW
        assert shape(ms, n, a, True)[0] == want_shape(n, a, True) != OK
    lo, hi = 1, SIZE_MAX // 32
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if sum(w for _, w in levels(mid, a)) <= SIZE_MAX // 32 else (lo, mid - 1)
    lv = levels(lo, a)
    assert shape(ms, lo, a, False) == (OK, len(lv) - 1, sum(w for _, w in lv)) and shape(ms, lo + 1, a, False)[0] == TREE_OVERFLOW
    for n in (lo - 1, lo, lo + 1, 3 * a ** 7, (1 << 62) + 1, 1 << 62):
        assert shape(ms, n, a, True)[0] == want_shape(n, a, True), n


@pytest.mark.parametrize("a", ARITIES)
def test_forest_bounds_on_both_sides(ms, a):
    """the 2-to-1 forest refuses n_trees > (SIZE_MAX / 128) / leaves_per_tree, the forest of any arity n_trees > (SIZE_MAX / 32) / tree_nodes"""
    for d in (0, 1, 3, 9):
        lpt = a ** d
        tree_nodes = sum(w for _, w in levels(lpt, a))
        for pair_bound, most in ((True, (SIZE_MAX // 128) // lpt), (False, (SIZE_MAX // 32) // tree_nodes)):
            for n_trees in (1, 2, 1000, most - 1, most):
                assert forest(ms, n_trees, lpt, a, pair_bound) == (OK, n_trees * lpt, n_trees * tree_nodes), (d, pair_bound, n_trees)
            for n_trees in (most + 1, 2 * most, SIZE_MAX):
                assert forest(ms, n_trees, lpt, a, pair_bound)[0] == FOREST_OVERFLOW, (d, pair_bound, n_trees)
            assert forest(ms, 0, lpt, a, pair_bound)[0] == NO_TREES
    # the tree's own shape comes first, in exact mode
    for pair_bound in (True, False):
        assert forest(ms, 0, 0, a, pair_bound)[0] == NO_LEAVES
        assert forest(ms, 0, a + 1, a, pair_bound)[0] == NOT_POWER and forest(ms, 4, 2 * a ** 2 + a, a, pair_bound)[0] == NOT_POWER
        big = a ** next(d for d in range(1, 65) if a ** (d + 1) > SIZE_MAX)
        assert forest(ms, 1, big, a, pair_bound)[0] == TREE_OVERFLOW


@pytest.mark.parametrize("a", list(ARITIES) + [255, 65536, 0xffffffff])
def test_arity_to_the_depth_in_64_bits(ms, a):
    last = next(d for d in range(65) if a ** (d + 1) > SIZE_MAX)       # the last depth that fits
    for d in (0, 1, 2, last - 1, last):
        assert leaves_of_depth(ms, a, d) == (OK, a ** d), d
    for d in (last + 1, last + 2, 64, 1000):
        if d > last:
            assert leaves_of_depth(ms, a, d)[0] == POW_OVERFLOW, d


# ---- the header under the sanitizers: a program of its own, nothing sanitized is loaded into this process --------------------------
def test_shape_header_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "merkle_shape_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", CSRC, os.path.join(HERE, "sanitize_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and "sanitized ok" in out.stdout, out.stdout + out.stderr
