"""squeeze_bytes / squeeze_bits of a batch (src/poseidon/mod.rs:256-286), the parts that need no device: the four entry points exist in
the header, both libraries, the ctypes table and the Rust declarations; the device conversion ABI residue -> canonical integer
(pmx_field.hpp: abi_to_canonical) and the position arithmetic of the conversion kernels (pmx_squeeze_cut.hpp), compiled for the host
(tests/squeeze_cut/squeeze_cut_host.cpp), against Python integers; the argument checks that come before a device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from sponge_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "squeeze_cut", "squeeze_cut_host.cpp")
NAMES = ["pmx_sponge_squeeze_bytes_batch", "pmx_sponge_squeeze_bytes_batch_dev", "pmx_sponge_squeeze_bits_batch",
         "pmx_sponge_squeeze_bits_batch_dev"]

BLS = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
BN254 = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
P25519 = (1 << 255) - 19
P248 = (1 << 248) - 237      # a 248-bit prime: u = 30 bytes / 247 bits
P226 = (1 << 226) - 5        # a 226-bit prime: u = 28 bytes / 225 bits, the smallest the library takes
MODULI = {"bls12_381_fr": BLS, "bn254_fr": BN254, "p25519": P25519, "p248": P248, "p226": P226}


@pytest.fixture(scope="module")
def sc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("squeeze_cut") / "libsqueeze_cut.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-DPMX_HOSTCHECK",
                           "-I", os.path.join(ROOT, "sponge_amd", "csrc"), SRC, "-o", out])
    lib = ctypes.CDLL(out)
    lib.sc_to_canonical.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.sc_to_canonical.restype = None
    lib.sc_unit.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.sc_unit.restype = ctypes.c_uint32
    lib.sc_elems.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    lib.sc_elems.restype = ctypes.c_uint64
    lib.sc_offset.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32]
    lib.sc_offset.restype = ctypes.c_uint64
    lib.sc_count.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32]
    lib.sc_count.restype = ctypes.c_uint32
    return lib


def test_the_four_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "poseidon_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    shipped, hooks = ctypes.CDLL(_lib.LIB_PATH), ctypes.CDLL(_lib.TEST_LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(shipped, name) and hasattr(hooks, name), name
        assert name in _lib.SIGNATURES, name
        assert f"fn {name}(" in ffi, name
    assert shipped.pmx_abi_version() == 5          # additive: the ABI version stays


def _limbs29(p):
    return np.array([(p >> (29 * i)) & ((1 << 29) - 1) for i in range(9)], dtype=np.uint32)


def _words32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint32)


def _canonical(sc, p, values):
    """abi_to_canonical of every 256-bit word of `values` (Python integers), as Python integers"""
    words = np.concatenate([_words32(v) for v in values]).copy()
    p29, p32 = _limbs29(p), _words32(p).copy()
    pinv = (-pow(p, -1, 1 << 29)) % (1 << 29)
    sc.sc_to_canonical(p29.ctypes.data, pinv, p32.ctypes.data, words.ctypes.data, len(values))
    raw = words.tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(values))]


@pytest.mark.parametrize("name", sorted(MODULI))
def test_conversion_to_the_canonical_integer_equals_python(sc, name):
    """a = x 2^256 mod p  ->  x in [0, p): into_bigint of ark-ff's Montgomery form.  The corner residues, 10^4 seeded ones, and
    unreduced words below 2^256 (the result is still the residue modulo p, fully reduced - pmx_field.hpp says so)."""
    p = MODULI[name]
    rinv = pow(1 << 256, -1, p)
    rng = np.random.default_rng(0x5C0E + p % 1000)
    rand = [int.from_bytes(rng.bytes(40), "little") for _ in range(10000)]
    reduced = [0, 1, p - 1, (1 << 256) % p, p // 2, (p - 1) // 3] + [v % p for v in rand]
    got = _canonical(sc, p, reduced)
    assert got == [a * rinv % p for a in reduced]
    assert all(0 <= x < p for x in got)
    unreduced = [p, p + 1, 2 * p, (1 << 256) - 1, (1 << 256) - p, ((1 << 256) // p) * p, 1 << 255] + [v % (1 << 256) for v in rand]
    got = _canonical(sc, p, unreduced)
    assert got == [a * rinv % p for a in unreduced]


@pytest.mark.parametrize("name,bits,unit_bytes", [("p226", 226, 28), ("p248", 248, 30), ("bn254_fr", 254, 31), ("bls12_381_fr", 255, 31),
                                                   ("p25519", 255, 31)])
def test_units_come_from_the_modulus_bit_length(sc, name, bits, unit_bytes):
    p = MODULI[name]
    assert p.bit_length() == bits
    p29 = _limbs29(p)
    assert sc.sc_unit(p29.ctypes.data, 0) == (bits - 1) // 8 == unit_bytes       # mod.rs:257
    assert sc.sc_unit(p29.ctypes.data, 1) == bits - 1                            # mod.rs:274


def _oracle_spans(length, unit):
    """mod.rs:256-286 as it is written: squeeze ceil(length / unit) elements, each yields `unit` units, truncate the concatenation.
    Returns E and, per element, (first, count) of the units that survive."""
    elems = (length + unit - 1) // unit
    produced = [(e * unit, unit) for e in range(elems)]
    return elems, [(first, min(first + cnt, length) - first) for first, cnt in produced]


@pytest.mark.parametrize("unit,top", [(28, 4 * 28 + 1), (31, 4 * 31 + 1), (224, 2 * 224 + 1), (254, 2 * 254 + 1)])
def test_packing_arithmetic_for_every_length(sc, unit, top):
    """E, every element's span in its row, the truncated tail: every num_bytes in 0 .. 4 u + 1 (u = 28, 31 bytes) and every num_bits in
    0 .. 2 u + 1 (u = 224, 254 bits); rows are packed, so the spans of consecutive elements tile the output without gap or overlap."""
    for length in range(top + 1):
        elems, spans = _oracle_spans(length, unit)
        assert sc.sc_elems(length, unit) == elems, (unit, length)
        for row in (0, 1, 7, (1 << 40) + 3):
            cursor = row * length
            for e, (first, count) in enumerate(spans):
                assert count >= 1
                assert sc.sc_offset(row, e, length, unit) == row * length + first == cursor, (unit, length, row, e)
                assert sc.sc_count(e, length, unit) == count, (unit, length, e)
                cursor += count
            assert cursor == (row + 1) * length == sc.sc_offset(row + 1, 0, length, unit)


def test_entry_points_reject_bad_arguments_without_a_device():
    """null context; null `out` with n * num_bytes > 0; n * num_bytes beyond size_t - all PMX_ERR_ARG before the context is read or a
    device is touched (the context handle below is never dereferenced)"""
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.uint64)
    tag = np.zeros(2, dtype=np.uint32)
    p, t = buf.ctypes.data, tag.ctypes.data
    fake = ctypes.c_void_p(p)
    for name in NAMES:
        fn = getattr(lib, name)
        tail = (None,) if name.endswith("_dev") else ()
        assert fn(None, p, t, t, p, 5, 2, *tail) == _lib.PMX_ERR_ARG, name
        assert b"null" in lib.pmx_last_error()
        assert fn(fake, p, t, t, None, 5, 2, *tail) == _lib.PMX_ERR_ARG, name
        assert b"null" in lib.pmx_last_error()
        assert fn(fake, None, t, t, p, 5, 2, *tail) == _lib.PMX_ERR_ARG, name
        assert fn(fake, p, t, t, p, (1 << 63) + 1, 2, *tail) == _lib.PMX_ERR_ARG, name
        assert b"overflows" in lib.pmx_last_error(), (name, lib.pmx_last_error())
        assert fn(fake, p, t, t, None, 0, 0, *tail) == _lib.PMX_OK, name        # nothing to do
