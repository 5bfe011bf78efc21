"""Matrix commitments (pmx_matrix_*), the parts that need no device:
- tests/matrix/matrix_host.cpp, a program of its own under ASan + UBSan over sponge_amd/csrc/pmx_matrix_shape.hpp: the slab walks, the
  strides of the two layouts, the 2-D copy geometry of a slab (performed with memcpy into a buffer of exactly the slab's size) and the
  byte-size refusals;
- the walk and the geometry, printed by that program, against plain Python arithmetic;
- the argument refusals of the shipped library that fire before a context is read, and pmx_matrix_rows - a host-only gather - against
  numpy for both layouts;
- the family is declared, exported by both libraries, bound in the ctypes table and the Rust declarations, adds no *_dev entry, and the
  header says what it lacks;
- the register report of hash_strided_kernel against hash_kernel on the two headline window engines (make asm1 ... EXTRA=-DPMX_ONE_MATRIX):
  no scratch, and no less occupancy."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sponge_amd import _lib
from sponge_amd.poseidon import matrix_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sponge_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "matrix", "matrix_host.cpp")
ROW, COL = _lib.MATRIX_ROW_MAJOR, _lib.MATRIX_COL_MAJOR
ENTRIES = ("pmx_matrix_leaves", "pmx_matrix_commit", "pmx_matrix_rows", "pmx_matrix_verify_rows")
HOOKS = ("pmx_test_matrix_slab_rows", "pmx_test_matrix_leaves_dev")


@pytest.fixture(scope="module")
def matrix_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("matrix") / "matrix_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", CSRC, SRC, "-o", exe])

    def run(*args):
        out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout
    return run


def test_host_pieces_under_asan_and_ubsan(matrix_host):
    assert "sanitized ok" in matrix_host()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_slab_walk_partitions_the_rows(matrix_host, n):
    for slab_rows in (1, 7, 64, n, n + 1):
        slabs = [tuple(int(x) for x in l.split()) for l in matrix_host("walk", str(n), str(slab_rows)).splitlines()]
        assert len(slabs) == -(-n // slab_rows)
        cursor = 0
        for s, (a, b) in enumerate(slabs):
            assert a == cursor and a < b <= n and b - a <= slab_rows
            assert b - a == slab_rows or s == len(slabs) - 1
            cursor = b
        assert cursor == n


@pytest.mark.parametrize("n,row_len,a,b", [(200, 5, 0, 200), (200, 5, 64, 128), (200, 5, 196, 200), (65, 1, 64, 65), (1 << 20, 64, 1 << 19, (1 << 19) + 4096)])
def test_copy_geometry_and_strides(matrix_host, n, row_len, a, b):
    col = [int(x) for x in matrix_host("copy", str(COL), str(n), str(row_len), str(a), str(b)).split()]
    assert col == [a * 32, n * 32, (b - a) * 32, (b - a) * 32, row_len, 1, b - a]
    row = [int(x) for x in matrix_host("copy", str(ROW), str(n), str(row_len), str(a), str(b)).split()]
    run = (b - a) * row_len * 32
    assert row == [a * row_len * 32, run, run, run, 1, row_len, 1]


# ---- the shipped library, no device ---------------------------------------------------------------------------------------------
def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_refusals_before_a_context_is_read():
    lib = _lib.lib()
    m = np.zeros((6, 4), dtype=np.uint64)
    out = np.full((40, 4), 0x77, dtype=np.uint64)
    idx = np.zeros(2, dtype=np.uint64)
    ok = np.full(2, 9, dtype=np.uint8)
    fake = _p(m)                                              # never dereferenced: every refusal below comes first
    big = 1 << 59
    cases = [
        (lib.pmx_matrix_leaves, (None, _p(m), 2, 3, COL, _p(out)), b"null"),
        (lib.pmx_matrix_leaves, (fake, None, 2, 3, COL, _p(out)), b"null"),
        (lib.pmx_matrix_leaves, (fake, _p(m), 2, 3, COL, None), b"null"),
        (lib.pmx_matrix_leaves, (fake, _p(m), 0, 3, COL, _p(out)), b"at least one row"),
        (lib.pmx_matrix_leaves, (fake, _p(m), 2, 0, COL, _p(out)), b"at least one element"),
        (lib.pmx_matrix_leaves, (fake, _p(m), 2, 3, 2, _p(out)), b"layout 2"),
        (lib.pmx_matrix_leaves, (fake, _p(m), big, 2, ROW, _p(out)), b"overflows"),
        (lib.pmx_matrix_commit, (None, _p(m), 2, 3, COL, 2, _p(out), _p(out)), b"null"),
        (lib.pmx_matrix_commit, (fake, None, 2, 3, COL, 2, _p(out), _p(out)), b"null"),
        (lib.pmx_matrix_commit, (fake, _p(m), 0, 3, COL, 2, _p(out), _p(out)), b"at least one row"),
        (lib.pmx_matrix_commit, (fake, _p(m), 2, 0, ROW, 2, _p(out), _p(out)), b"at least one element"),
        (lib.pmx_matrix_commit, (fake, _p(m), 2, 3, 2, 2, _p(out), _p(out)), b"layout 2"),
        (lib.pmx_matrix_commit, (fake, _p(m), 2, big, COL, 2, _p(out), _p(out)), b"overflows"),
        (lib.pmx_matrix_commit, (fake, _p(m), (1 << 59) - 1, 1, COL, 2, _p(out), _p(out)), b"too large"),     # the bytes fit, the launch grid does not
        (lib.pmx_matrix_commit, (fake, _p(m), 2, 3, COL, 1, _p(out), _p(out)), b"arity"),
        (lib.pmx_matrix_rows, (None, 2, 3, COL, _p(idx), 2, _p(out)), b"null"),
        (lib.pmx_matrix_rows, (_p(m), 2, 3, COL, None, 2, _p(out)), b"null"),
        (lib.pmx_matrix_rows, (_p(m), 2, 3, COL, _p(idx), 2, None), b"null"),
        (lib.pmx_matrix_rows, (_p(m), 0, 3, COL, _p(idx), 2, _p(out)), b"at least one row"),
        (lib.pmx_matrix_rows, (_p(m), 2, 0, COL, _p(idx), 2, _p(out)), b"at least one element"),
        (lib.pmx_matrix_rows, (_p(m), 2, 3, 2, _p(idx), 2, _p(out)), b"layout 2"),
        (lib.pmx_matrix_rows, (_p(m), big, 2, COL, _p(idx), 2, _p(out)), b"overflows"),
        (lib.pmx_matrix_verify_rows, (None, _p(m), 3, _p(idx), _p(out), 1, 2, 2, 2, _p(out), _p(ok)), b"null"),
        (lib.pmx_matrix_verify_rows, (fake, None, 3, _p(idx), _p(out), 1, 2, 2, 2, _p(out), _p(ok)), b"null"),
        (lib.pmx_matrix_verify_rows, (fake, _p(m), 3, None, _p(out), 1, 2, 2, 2, _p(out), _p(ok)), b"null"),
        (lib.pmx_matrix_verify_rows, (fake, _p(m), 3, _p(idx), None, 1, 2, 2, 2, _p(out), _p(ok)), b"null"),
        (lib.pmx_matrix_verify_rows, (fake, _p(m), 3, _p(idx), _p(out), 1, 2, 2, 2, None, _p(ok)), b"null"),
        (lib.pmx_matrix_verify_rows, (fake, _p(m), 3, _p(idx), _p(out), 1, 2, 2, 2, _p(out), None), b"null"),
        (lib.pmx_matrix_verify_rows, (fake, _p(m), 0, _p(idx), _p(out), 1, 2, 2, 2, _p(out), _p(ok)), b"at least one element"),
        (lib.pmx_matrix_verify_rows, (fake, _p(m), 3, _p(idx), _p(out), 1, 2, 0, 2, _p(out), _p(ok)), b"at least one leaf"),
        (lib.pmx_matrix_verify_rows, (fake, _p(m), 3, _p(idx), _p(out), 1, 1, 2, 2, _p(out), _p(ok)), b"arity"),
        (lib.pmx_matrix_verify_rows, (fake, _p(m), 3, _p(idx), _p(out), 3, 2, 2, 2, _p(out), _p(ok)), b"depth 3 is not the depth 1"),
    ]
    for fn, args, needle in cases:
        assert fn(*args) == _lib.PMX_ERR_ARG, (fn.__name__, args)
        assert needle in lib.pmx_last_error(), (fn.__name__, needle, lib.pmx_last_error())
    assert (out == 0x77).all() and (ok == 9).all(), "a refusal wrote a result"


def _matrix(n_rows, row_len, layout, seed=5):
    """(flat matrix in the layout, the same as [n_rows][row_len][4])"""
    rows = np.random.default_rng(seed).integers(0, 1 << 63, (n_rows, row_len, 4)).astype(np.uint64)
    flat = rows if layout == ROW else np.ascontiguousarray(rows.transpose(1, 0, 2))
    return np.ascontiguousarray(flat).reshape(-1, 4), rows


@pytest.mark.parametrize("layout", [ROW, COL])
@pytest.mark.parametrize("n_rows,row_len", [(1, 1), (7, 3), (3, 7), (64, 17)])
def test_matrix_rows_is_the_numpy_gather(layout, n_rows, row_len):
    flat, rows = _matrix(n_rows, row_len, layout)
    idx = np.array([n_rows - 1, 0, n_rows // 2, n_rows - 1], dtype=np.uint64)
    assert np.array_equal(matrix_rows(flat, n_rows, row_len, layout, idx), rows[idx.astype(np.int64)])
    assert matrix_rows(flat, n_rows, row_len, layout, []).shape == (0, row_len, 4)


@pytest.mark.parametrize("layout", [ROW, COL])
def test_matrix_rows_checks_every_index_before_it_writes(layout):
    flat, _ = _matrix(7, 3, layout)
    out = np.full((3, 3, 4), 0x55, dtype=np.uint64)
    for bad in (7, (1 << 64) - 1):
        idx = np.array([0, 1, bad], dtype=np.uint64)          # the bad index is the LAST one: the first two rows must not have been written
        assert _lib.lib().pmx_matrix_rows(_p(flat), 7, 3, layout, _p(idx), 3, _p(out)) == _lib.PMX_ERR_ARG
        assert b"out of range" in _lib.lib().pmx_last_error()
        assert (out == 0x55).all()


def test_the_family_is_declared_exported_and_bound_and_adds_no_dev_entry():
    header = open(os.path.join(ROOT, "include", "poseidon_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES
        for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    assert re.search(r"#define PMX_MATRIX_ROW_MAJOR 0u", code) and re.search(r"#define PMX_MATRIX_COL_MAJOR 1u", code)
    assert re.search(r"#define PMX_MATRIX_SLAB_BYTES ", code)
    assert not re.search(r"\bpmx_matrix_\w*_dev\b", header)
    assert len(set(re.findall(r"\b(pmx_\w+_dev)\s*\(", code))) == 25        # the device entry points are what they were
    assert "no device-resident form" in header and "no forest of matrices" in header and "no device-group form" in header
    testing = open(os.path.join(ROOT, "include", "poseidon_mi355x_testing.h")).read()
    for hook in HOOKS:
        assert re.search(r"\b" + hook + r"\s*\(", testing) and hook in _lib.TEST_HOOK_SIGNATURES
        assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), hook)                # the hooks exist in the test library only
        assert hasattr(ctypes.CDLL(_lib.TEST_LIB_PATH), hook)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in ENTRIES:
        assert f"fn {name}(" in ffi, name
    assert "PMX_MATRIX_COL_MAJOR: u32 = 1" in ffi and "PMX_MATRIX_ROW_MAJOR: u32 = 0" in ffi
    mod = open(os.path.join(ROOT, "bindings", "rust", "src", "mod.rs")).read()
    assert "pub fn matrix_commit(" in mod and "pub fn matrix_verify_rows(" in mod
    assert _lib.lib().pmx_abi_version() == 5                                # additive: the ABI version stays


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
@pytest.mark.parametrize("t", [3, 9])
def test_strided_kernel_keeps_the_hash_kernels_occupancy_without_scratch(t):
    subprocess.check_call(["make", "-C", CSRC, "asm1", f"T={t}", "ALPHA=5", "EXTRA=-DPMX_ONE_MATRIX"], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    rpt = open(os.path.join(CSRC, "build", f"one_t{t}.rpt")).read()
    blocks = {m.group(1): m.group(2) for m in re.finditer(r"Function Name: (\S+)(.*?)(?=Function Name: |\Z)", rpt, flags=re.S)}
    get = lambda block, key: int(re.search(key + r": (\d+)", block).group(1))
    occupancy = {}
    for kernel in ("hash_strided_kernel", "hash_kernel"):
        names = [n for n in blocks if re.search(r"\d+" + kernel + "I", n) and f"HybridEngineILi{t}ELi5EEE" in n]
        assert len(names) == 1, (kernel, sorted(blocks))
        block = blocks[names[0]]
        assert get(block, r"ScratchSize \[bytes/lane\]") == 0, block
        occupancy[kernel] = get(block, r"Occupancy \[waves/SIMD\]")
    assert occupancy["hash_strided_kernel"] >= occupancy["hash_kernel"] >= 1, occupancy
