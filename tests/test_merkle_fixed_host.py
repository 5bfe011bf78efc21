"""Trees of a fixed depth (pmx_merkle_fixed*, pmx_merkle_frontier_append), the parts that need no device:
- tests/merkle_fixed/frontier_host.cpp, a program of its own under ASan + UBSan over sponge_amd/csrc/pmx_merkle_frontier.hpp: for k in
  {2, 3, 8}, every depth with k^D <= 4096 and every (n, m) with n + m <= k^D the row counts per level, the partial node's position, the
  pads, the frontier digits, and the walk replayed on the plan's own lists (no slot is read before it is placed); k^D = 2^64 at (2, 64),
  refusal at (2, 65) and (3, 41);
- plans printed by that program against plain Python arithmetic;
- the oracle's two ways to a tree - literally padded, and the populated part over the default chain - agree;
- the refusals of the shipped library that fire before a context is read: each returns its status and writes nothing;
- pmx_merkle_fixed_shape and pmx_merkle_fixed_paths, host-only, against the oracle;
- the family is declared, exported by both libraries, bound in the ctypes table and the Rust declarations, adds no *_dev entry, and the
  ABI version is still 5."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from sponge_amd import _lib
from sponge_amd.poseidon import merkle_fixed_paths, merkle_fixed_shape

import merkle_ary_oracle as MA
import merkle_fixed_oracle as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sponge_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "merkle_fixed", "frontier_host.cpp")
ENTRIES = ("pmx_merkle_fixed_defaults", "pmx_merkle_frontier_append", "pmx_merkle_fixed_shape", "pmx_merkle_fixed", "pmx_merkle_fixed_paths")
HOOK = "pmx_test_merkle_fixed_piece"


@pytest.fixture(scope="module")
def frontier_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_fixed") / "frontier_host")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-pthread", "-I", CSRC, SRC, "-o", exe])

    def run(*args):
        out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout
    return run


def test_index_arithmetic_under_asan_and_ubsan(frontier_host):
    assert "sanitized ok" in frontier_host()


def _plan(n, m, k, depth):
    """(first, kept, fresh, partial, pads, parents, digit, digit_slot) per level by plain arithmetic"""
    out, total = [], n + m
    for l in range(depth + 1):
        f, g = n // k ** l, total // k ** l
        partial = 1 if total % k ** l else 0
        if l == depth:
            out.append((0, 0, g - f, partial, 0, 0, 0, 0))
            break
        kept, rows = f % k, f % k + g - f + partial
        parents = -(-rows // k)
        out.append((f - kept, kept, g - f, partial, parents * k - rows, parents, g % k, (g - g % k) - (f - kept)))
    return out


@pytest.mark.parametrize("n,m,k,depth", [(0, 0, 2, 4), (5, 6, 2, 4), (15, 1, 2, 4), (16, 0, 2, 4), (26, 1, 3, 3), (1000, 300, 2, 32), (1000, 300, 8, 21),
                                         (8 ** 7 - 1, 1, 8, 21), (2 ** 64 - 2, 1, 2, 64), (12345678901234567, 4096, 3, 40)])
def test_printed_plans_are_the_arithmetic(frontier_host, n, m, k, depth):
    lines = [tuple(int(x) for x in l.split()) for l in frontier_host("plan", str(n), str(m), str(k), str(depth)).splitlines()]
    assert [l[:8] for l in lines] == _plan(n, m, k, depth)
    # the rows lie one behind the other, behind the uploaded and the downloaded block
    cursor = 2 * depth * (k - 1) + depth + 2
    for l, line in enumerate(lines):
        assert line[8] == cursor
        cursor += line[5] * k if l < depth else 1


def test_refused_shapes_print_no_plan(frontier_host):
    for args in (("0", "1", "2", "65"), ("0", "1", "3", "41"), ("16", "1", "2", "4"), ("0", "1", "1", "4"), ("0", "1", "2", "0")):
        assert frontier_host("plan", *args).startswith("refused")


@pytest.mark.parametrize("label,a,depth", [("t3", 2, 4), ("t9-bn254", 3, 3), ("t9-bn254", 8, 2)])
def test_the_oracles_two_ways_agree(label, a, depth):
    _, _, cr = M.config(label)
    e = M.cached_defaults(label, a, depth)
    for n in range(a ** depth + 1):
        full = M.cached_padded(label, a, depth, n)
        part = M.sparse_levels(cr, M.leaf_row(label, a ** depth)[:n], a, depth, e)
        for l in range(depth + 1):
            assert np.array_equal(full[l][:part[l].shape[0]], part[l]) and part[l].shape[0] == -(-n // a ** l)
            assert (full[l][part[l].shape[0]:] == e[l]).all()          # everything beyond the populated part is the default digest
        assert np.array_equal(M.root_of(part, e, depth), full[depth][0])


# ---- the shipped library, no device ---------------------------------------------------------------------------------------------
def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_refusals_before_a_context_is_read():
    lib = _lib.lib()
    leaves = np.zeros((8, 4), dtype=np.uint64)
    out = np.full((200, 4), 0x77, dtype=np.uint64)
    n_nodes = ctypes.c_size_t(0x77)
    idx = np.zeros(2, dtype=np.uint64)
    fake = _p(leaves)                                         # never dereferenced: every refusal below comes first
    o, d, f = _p(out), _p(leaves), _p(leaves)
    big = 1 << 61
    cases = [
        (lib.pmx_merkle_fixed_defaults, (None, d, 2, 4, o), b"null"),
        (lib.pmx_merkle_fixed_defaults, (fake, None, 2, 4, o), b"null"),
        (lib.pmx_merkle_fixed_defaults, (fake, d, 2, 4, None), b"null"),
        (lib.pmx_merkle_fixed_defaults, (fake, d, 1, 4, o), b"arity"),
        (lib.pmx_merkle_fixed_defaults, (fake, d, 2, 0, o), b"depth"),
        (lib.pmx_merkle_fixed_defaults, (fake, d, 2, 65, o), b"depth"),
        (lib.pmx_merkle_fixed_defaults, (fake, d, 3, 41, o), b"overflows 64 bits"),
        (lib.pmx_merkle_frontier_append, (None, 2, 4, d, f, 3, d, 2, o, o), b"null"),
        (lib.pmx_merkle_frontier_append, (fake, 2, 4, None, f, 3, d, 2, o, o), b"null"),
        (lib.pmx_merkle_frontier_append, (fake, 2, 4, d, None, 3, d, 2, o, o), b"null"),          # frontier_in may be NULL only at n_leaves = 0
        (lib.pmx_merkle_frontier_append, (fake, 2, 4, d, f, 3, None, 2, o, o), b"null"),
        (lib.pmx_merkle_frontier_append, (fake, 2, 4, d, f, 3, d, 2, None, o), b"null"),
        (lib.pmx_merkle_frontier_append, (fake, 1, 4, d, f, 3, d, 2, o, o), b"arity"),
        (lib.pmx_merkle_frontier_append, (fake, 2, 0, d, f, 3, d, 2, o, o), b"depth"),
        (lib.pmx_merkle_frontier_append, (fake, 2, 65, d, f, 3, d, 2, o, o), b"depth"),
        (lib.pmx_merkle_frontier_append, (fake, 3, 41, d, f, 3, d, 2, o, o), b"overflows 64 bits"),
        (lib.pmx_merkle_frontier_append, (fake, 2, 4, d, f, 15, d, 2, o, o), b"more leaves"),
        (lib.pmx_merkle_frontier_append, (fake, 2, 4, d, f, 17, d, 0, o, o), b"more leaves"),
        (lib.pmx_merkle_frontier_append, (fake, 3, 3, d, f, 27, d, 1, o, o), b"more leaves"),
        (lib.pmx_merkle_frontier_append, (fake, 2, 64, d, f, (1 << 64) - 1, d, 1, o, o), b"more leaves"),
        (lib.pmx_merkle_frontier_append, (fake, 2, 64, d, f, 3, d, big, o, o), b"overflows size_t"),
        (lib.pmx_merkle_frontier_append, (fake, 2, 4, d, f, 16, d, 0, o, o), b"full tree"),       # (root NULL would be accepted)
        (lib.pmx_merkle_fixed_shape, (3, 2, 4, None), b"null"),
        (lib.pmx_merkle_fixed_shape, (0, 2, 4, ctypes.byref(n_nodes)), b"at least one leaf"),
        (lib.pmx_merkle_fixed_shape, (17, 2, 4, ctypes.byref(n_nodes)), b"more leaves"),
        (lib.pmx_merkle_fixed_shape, (3, 1, 4, ctypes.byref(n_nodes)), b"arity"),
        (lib.pmx_merkle_fixed_shape, (3, 2, 0, ctypes.byref(n_nodes)), b"depth"),
        (lib.pmx_merkle_fixed_shape, (3, 2, 65, ctypes.byref(n_nodes)), b"depth"),
        (lib.pmx_merkle_fixed_shape, (3, 3, 41, ctypes.byref(n_nodes)), b"overflows 64 bits"),
        (lib.pmx_merkle_fixed_shape, (big, 2, 64, ctypes.byref(n_nodes)), b"overflows size_t"),
        (lib.pmx_merkle_fixed, (None, d, 3, 2, 4, d, o, o), b"null"),
        (lib.pmx_merkle_fixed, (fake, None, 3, 2, 4, d, o, o), b"null"),
        (lib.pmx_merkle_fixed, (fake, d, 3, 2, 4, None, o, o), b"null"),
        (lib.pmx_merkle_fixed, (fake, d, 0, 2, 4, d, o, o), b"at least one leaf"),
        (lib.pmx_merkle_fixed, (fake, d, 17, 2, 4, d, o, o), b"more leaves"),
        (lib.pmx_merkle_fixed, (fake, d, 3, 1, 4, d, o, o), b"arity"),
        (lib.pmx_merkle_fixed, (fake, d, 3, 2, 65, d, o, o), b"depth"),
        (lib.pmx_merkle_fixed, (fake, d, 3, 3, 41, d, o, o), b"overflows 64 bits"),
        (lib.pmx_merkle_fixed_paths, (None, 3, 2, 4, d, _p(idx), 2, o), b"null"),
        (lib.pmx_merkle_fixed_paths, (d, 3, 2, 4, None, _p(idx), 2, o), b"null"),
        (lib.pmx_merkle_fixed_paths, (d, 3, 2, 4, d, None, 2, o), b"null"),
        (lib.pmx_merkle_fixed_paths, (d, 3, 2, 4, d, _p(idx), 2, None), b"null"),
        (lib.pmx_merkle_fixed_paths, (d, 0, 2, 4, d, _p(idx), 2, o), b"at least one leaf"),
        (lib.pmx_merkle_fixed_paths, (d, 17, 2, 4, d, _p(idx), 2, o), b"more leaves"),
        (lib.pmx_merkle_fixed_paths, (d, 3, 2, 0, d, _p(idx), 2, o), b"depth"),
    ]
    for fn, args, needle in cases:
        assert fn(*args) == _lib.PMX_ERR_ARG, (fn.__name__, args)
        assert needle in lib.pmx_last_error(), (fn.__name__, needle, lib.pmx_last_error())
    assert (out == 0x77).all() and n_nodes.value == 0x77, "a refusal wrote a result"


@pytest.mark.parametrize("a,depth", [(2, 4), (3, 3), (8, 2), (2, 64), (8, 21)])
def test_fixed_shape_is_the_sum_of_the_stored_widths(a, depth):
    for n in [1, 2, a - 1, a, a + 1, 1000, a ** depth - 1, a ** depth]:
        if 1 <= n <= min(a ** depth, 1 << 40):
            assert merkle_fixed_shape(n, a, depth) == sum(M.widths(n, a, depth)), (n, a, depth)


@pytest.mark.parametrize("label,a,depth,n", [("t3", 2, 4, 1), ("t3", 2, 4, 11), ("t3", 2, 4, 16), ("t9-bn254", 3, 3, 14), ("t9-bn254", 8, 2, 9)])
def test_fixed_paths_gather_is_host_only_and_climbs_to_the_oracle_root(label, a, depth, n):
    """pmx_merkle_fixed_paths over a dense array built by the oracle (no device involved): every sibling is the node or the default digest
    the index arithmetic says, and the oracle's climb of a tree of a^depth leaves reaches the root."""
    _, _, cr = M.config(label)
    e = M.cached_defaults(label, a, depth)
    levels = M.cached_padded(label, a, depth, n)
    nodes = M.dense_of(levels, n, a, depth)
    idx = np.array(sorted({0, n - 1, n // 2}), dtype=np.uint64)
    paths = merkle_fixed_paths(nodes, n, a, depth, e, idx)
    assert np.array_equal(paths, M.open_paths(levels, n, a, depth, e, idx))
    assert np.array_equal(paths, MA.open_paths(np.concatenate(levels), a ** depth, a, idx))     # the openings of the padded tree
    tops = MA.climb(cr, levels[0][idx.astype(np.int64)], idx, paths, a)
    assert all(np.array_equal(top, levels[depth][0]) for top in tops)
    # every index is checked before anything is written
    out = np.full((3, depth, a - 1, 4), 0x55, dtype=np.uint64)
    for bad in (n, (1 << 64) - 1):
        bad_idx = np.array([0, 0, bad], dtype=np.uint64)
        assert _lib.lib().pmx_merkle_fixed_paths(_p(nodes), n, a, depth, _p(np.ascontiguousarray(e)), _p(bad_idx), 3, _p(out)) == _lib.PMX_ERR_ARG
        assert b"out of range" in _lib.lib().pmx_last_error() and (out == 0x55).all()


def test_the_family_is_declared_exported_and_bound_and_adds_no_dev_entry():
    header = open(os.path.join(ROOT, "include", "poseidon_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES
        for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    assert not re.search(r"\bpmx_merkle_fixed\w*_dev\b", header) and not re.search(r"\bpmx_merkle_frontier\w*_dev\b", header)
    assert len(set(re.findall(r"\b(pmx_\w+_dev)\s*\(", code))) == 25        # the device entry points are what they were
    for sentence in ("no device-resident form", "no forest of matrices", "no device-group form", "no *_dev entry"):
        assert sentence in header
    testing = open(os.path.join(ROOT, "include", "poseidon_mi355x_testing.h")).read()
    assert re.search(r"\b" + HOOK + r"\s*\(", testing) and HOOK in _lib.TEST_HOOK_SIGNATURES
    assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), HOOK) and hasattr(ctypes.CDLL(_lib.TEST_LIB_PATH), HOOK)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in ENTRIES:
        assert f"fn {name}(" in ffi, name
    mod = open(os.path.join(ROOT, "bindings", "rust", "src", "mod.rs")).read()
    assert "pub fn merkle_frontier_append(" in mod and "pub fn merkle_fixed(" in mod and "pub fn merkle_fixed_defaults(" in mod
    assert "class IncrementalMerkleTree" in open(os.path.join(ROOT, "sponge_amd", "host", "poseidon_sponge.hpp")).read()
    assert _lib.lib().pmx_abi_version() == 5                                # additive: the ABI version stays
