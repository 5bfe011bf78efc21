"""Proof-of-work grinding (pmx_sponge_grind), the parts that need no device:
- tests/grind/grind_host.cpp, a program of its own under ASan + UBSan: the integer -> ABI residue conversion of pmx_field.hpp
  (abi_from_u64, what grind_kernel absorbs per candidate) against the host field code behind pmx_to_mont, the acceptance test on the
  canonical digest, and the chunk walk of the host loop (pmx_grind_plan.hpp);
- the same conversion, printed by that program, against pmx_to_mont through the library on BLS12-381 Fr and BN254 Fr;
- the chunk walk, printed by that program, against plain Python arithmetic;
- the register report of grind_kernel on the two headline window engines (make asm1 ... EXTRA=-DPMX_ONE_GRIND): no scratch, and the
  occupancy of the permute kernel of the same engine;
- the entry is declared, exported by both libraries, bound in the ctypes table and the Rust declarations, and adds no *_dev entry;
- the argument checks that fire before a context is read."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sponge_amd as S
from sponge_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sponge_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "grind", "grind_host.cpp")
CORNERS = [0, 1, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1]


@pytest.fixture(scope="module")
def grind_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grind") / "grind_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Wno-unknown-pragmas", "-DPMX_HOSTCHECK", "-I", CSRC, SRC, "-o", exe])

    def run(*args):
        out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout
    return run


def test_host_pieces_under_asan_and_ubsan(grind_host):
    assert "sanitized ok" in grind_host()


def test_integer_to_residue_equals_pmx_to_mont(grind_host):
    """abi_from_u64(v) = v * 2^256 mod p, fully reduced: limb for limb what pmx_to_mont makes of the canonical integer v - F::from(v)"""
    lines = [l.split() for l in grind_host("residues").splitlines()]
    assert len(lines) == 2 * len(CORNERS)
    for field in (S.BLS12_381_FR, S.BN254_FR):
        mine = {int(v): int(r, 16) for name, v, r in lines if name == field.name}
        assert sorted(mine) == CORNERS
        want = field.from_ints(CORNERS)                       # pmx_to_mont
        for v, row in zip(CORNERS, want):
            assert mine[v] == sum(int(row[i]) << (64 * i) for i in range(4)), (field.name, v)
            assert mine[v] == v * (1 << 256) % field.modulus


@pytest.mark.parametrize("first,count,chunk", [
    (0, 1, 1 << 20), (5, 300, 1 << 20),                       # count below one chunk
    (0, 1 << 16, 1 << 16), (9, (1 << 16) + 1, 1 << 16),       # exactly one chunk; one candidate into the second
    (3, 1001, 64), ((1 << 32) - 100, 300, 128),
    ((1 << 64) - 300, 300, 64), ((1 << 64) - 300, 300, 1 << 20), ((1 << 64) - 1, 1, 1 << 20),   # first + count = 2^64
    (0, 0, 1 << 20), ((1 << 64) - 1, 0, 64),                  # empty
])
def test_chunk_walk_is_ascending_disjoint_and_exact(grind_host, first, count, chunk):
    chunks = [tuple(int(x) for x in l.split()) for l in grind_host("walk", str(first), str(count), str(chunk)).splitlines()]
    assert len(chunks) == -(-count // chunk)
    cursor = first
    for k, (f, c) in enumerate(chunks):
        assert f == cursor and 1 <= c <= chunk and f + c <= 1 << 64
        assert c == chunk or k == len(chunks) - 1
        cursor = f + c
    assert cursor == first + count


@pytest.mark.parametrize("first,count", [((1 << 64) - 299, 300), ((1 << 64) - 1, 2), (2, (1 << 64) - 1)])
def test_chunk_walk_refuses_a_range_beyond_2_64(grind_host, first, count):
    assert grind_host("walk", str(first), str(count), "64").strip() == "refused"


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
@pytest.mark.parametrize("t,waves", [(3, 4), (9, 2)])
def test_grind_kernel_keeps_the_permute_kernels_occupancy_without_scratch(t, waves):
    subprocess.check_call(["make", "-C", CSRC, "asm1", f"T={t}", "ALPHA=5", "EXTRA=-DPMX_ONE_GRIND"], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    rpt = open(os.path.join(CSRC, "build", f"one_t{t}.rpt")).read()
    blocks = {m.group(1): m.group(2) for m in re.finditer(r"Function Name: (\S+)(.*?)(?=Function Name: |\Z)", rpt, flags=re.S)}
    get = lambda block, key: int(re.search(key + r": (\d+)", block).group(1))
    occupancy = {}
    for kernel in ("grind_kernel", "permute_kernel"):
        names = [n for n in blocks if kernel in n and f"HybridEngineILi{t}ELi5EEE" in n]
        assert len(names) == 1, (kernel, sorted(blocks))
        block = blocks[names[0]]
        assert get(block, r"ScratchSize \[bytes/lane\]") == 0, block
        occupancy[kernel] = get(block, r"Occupancy \[waves/SIMD\]")
    assert occupancy["grind_kernel"] >= occupancy["permute_kernel"] >= waves, occupancy


def test_the_entry_is_declared_exported_and_bound_and_adds_no_dev_entry():
    header = open(os.path.join(ROOT, "include", "poseidon_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bpmx_sponge_grind\s*\(", code) and re.search(r"#define PMX_OP_GRIND 5\b", code)
    assert not re.search(r"\bpmx_sponge_grind\w*_dev\b", header)
    assert len(set(re.findall(r"\b(pmx_\w+_dev)\s*\(", code))) == 25        # the device entry points are what they were
    assert "no *_dev entry" in header                                       # and the header says what the family lacks
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), "pmx_sponge_grind"), path
    assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), "pmx_test_grind_chunk")  # the chunk hook exists in the test library only
    assert hasattr(ctypes.CDLL(_lib.TEST_LIB_PATH), "pmx_test_grind_chunk")
    assert "pmx_sponge_grind" in _lib.SIGNATURES and _lib.OP_GRIND == 5
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert "fn pmx_sponge_grind(" in ffi and "PMX_OP_GRIND: c_int = 5" in ffi
    assert "pub fn grind(" in open(os.path.join(ROOT, "bindings", "rust", "src", "mod.rs")).read()
    assert _lib.lib().pmx_abi_version() == 5                                # additive: the ABI version stays


def test_null_pointers_are_refused_before_a_context_is_read():
    lib = _lib.lib()
    state = np.zeros(12, dtype=np.uint64)
    nonce, found = ctypes.c_uint64(0x77), ctypes.c_int(5)
    p, n, f = ctypes.c_void_p(state.ctypes.data), ctypes.byref(nonce), ctypes.byref(found)
    fake = ctypes.c_void_p(state.ctypes.data)                               # never dereferenced: a null pointer is found first
    for args in ((None, p, 0, 0, 6, 0, 10, n, f), (fake, None, 0, 0, 6, 0, 10, n, f), (fake, p, 0, 0, 6, 0, 10, None, f),
                 (fake, p, 0, 0, 6, 0, 10, n, None)):
        assert lib.pmx_sponge_grind(*args) == _lib.PMX_ERR_ARG
        assert b"null" in lib.pmx_last_error()
    assert nonce.value == 0x77 and found.value == 5
