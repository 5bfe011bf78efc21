"""The device-resident matrix entries (include/poseidon_mi355x_resident.h), the parts that need no device:
- the five functions are declared in the header of their own, exported by both libraries and bound through _lib.RESIDENT_SIGNATURES,
  which shares no name with _lib.SIGNATURES; the main header, the ABI version and the Rust declarations are what they were;
- pmx_matrix_view_extent against plain Python arithmetic: the views a caller has (packed and pitched row-major, column-major with
  ld = n_rows and ld > n_rows, 1 x 1, a block of a larger matrix), the refusals, and the overflow boundary from both sides;
- the refusals of the four stream-taking entries that fire before a context is read.
The gather's own index arithmetic is one line inside matrix_rows_kernel (pmx_tree_moves.hip) over a view this function has accepted; it
has no host twin to compile, and tests/test_gpu_matrix_resident.py runs it."""
import ctypes
import os
import re

import numpy as np
import pytest

from sponge_amd import _lib
from sponge_amd.merkle import matrix_view_extent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pmx_matrix_view_extent", "pmx_matrix_leaves_dev", "pmx_matrix_commit_dev", "pmx_matrix_open_dev", "pmx_matrix_verify_rows_dev")
SIZE_MAX = (1 << 64) - 1
LIMIT = SIZE_MAX // 32                     # the most elements whose bytes fit size_t


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"\b(pmx_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))


def test_the_entries_are_declared_exported_and_bound_through_a_table_of_their_own():
    assert declared("poseidon_mi355x_resident.h") == sorted(ENTRIES) == sorted(_lib.RESIDENT_SIGNATURES)
    assert not set(_lib.RESIDENT_SIGNATURES) & set(_lib.SIGNATURES)
    assert not set(_lib.RESIDENT_SIGNATURES) & (set(_lib.TEST_HOOK_SIGNATURES) | set(_lib.DIAG_SIGNATURES))
    assert sorted(_lib.SIGNATURES) == declared("poseidon_mi355x.h")                     # the main table is the main header's, as before
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        handle = ctypes.CDLL(path)
        for name in ENTRIES:
            assert hasattr(handle, name), (path, name)
    assert not any(hasattr(ctypes.CDLL(_lib.DIAG_LIB_PATH), name) for name in ENTRIES)
    lib = _lib.lib()
    for name, (restype, argtypes) in _lib.RESIDENT_SIGNATURES.items():                  # lib() has bound them
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert lib.pmx_abi_version() == _lib.ABI_VERSION == 5
    resident = open(os.path.join(ROOT, "include", "poseidon_mi355x_resident.h")).read()
    assert '#include "poseidon_mi355x.h"' in resident and "PMX_ABI_VERSION" not in resident
    assert "unspecified" in resident and "captured" in resident.lower()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert not any(f"fn {name}(" in ffi for name in ENTRIES)                            # the Rust binding is out of scope


def want_extent(n_rows, row_len, row_stride, elem_stride):
    """the header's sentence: None where it refuses"""
    if n_rows == 0 or row_len == 0 or row_stride == 0 or elem_stride == 0:
        return None
    extent = 1 + (n_rows - 1) * row_stride + (row_len - 1) * elem_stride
    return extent if extent * 32 <= SIZE_MAX else None


def got_extent(*view):
    out = ctypes.c_size_t(0xDEAD)
    rc = _lib.lib().pmx_matrix_view_extent(*view, ctypes.byref(out))
    if rc == _lib.PMX_OK:
        return out.value
    assert rc == _lib.PMX_ERR_ARG and out.value == 0xDEAD, (view, rc, out.value)
    return None


VIEWS = [
    (7, 3, 3, 1), (257, 17, 17, 1),                            # packed row-major
    (7, 3, 6, 1), (257, 17, 20, 1),                            # pitched row-major
    (7, 3, 1, 7), (257, 17, 1, 257),                           # column-major, ld = n_rows
    (7, 3, 1, 10), (257, 17, 1, 260),                          # column-major, ld > n_rows
    (1, 1, 1, 1), (1, 1, 9, 11), (1, 5, 1, 1), (5, 1, 1, 1),   # 1 x 1 whatever the strides; one row; one column
    (64, 8, 1, 1 << 20), (64, 8, 1 << 20, 1),                  # a block of a larger matrix
    (4, 4, 1, 1),                                              # overlapping elements: legal, the matrix is only read
    (0, 3, 3, 1), (7, 0, 3, 1), (7, 3, 0, 1), (7, 3, 3, 0), (0, 0, 0, 0), (1, 1, 0, 1), (1, 1, 1, 0),
]


@pytest.mark.parametrize("view", VIEWS)
def test_view_extent_is_the_headers_arithmetic(view):
    want = want_extent(*view)
    assert got_extent(*view) == want
    if want is None:
        with pytest.raises(_lib.PmxError):
            matrix_view_extent(*view)
    else:
        assert matrix_view_extent(*view) == want


def test_view_extent_at_the_overflow_boundary():
    """the largest accepted extent is LIMIT = floor(SIZE_MAX / 32) elements; one more is refused, however the view reaches it"""
    assert LIMIT == (1 << 59) - 1
    for accepted, refused in [((LIMIT, 1, 1, 1), (LIMIT + 1, 1, 1, 1)),                 # one column of LIMIT rows
                              ((1, LIMIT, 1, 1), (1, LIMIT + 1, 1, 1)),                 # one row
                              ((2, 1, LIMIT - 1, 1), (2, 1, LIMIT, 1)),                 # two rows, the stride carries it
                              ((1, 2, 1, LIMIT - 1), (1, 2, 1, LIMIT)),
                              ((3, 2, (LIMIT - 2) // 2, 1 + (LIMIT - 2) % 2), (3, 2, (LIMIT - 2) // 2, 2 + (LIMIT - 2) % 2)),    # both terms
                              ((1 << 29, 1 << 29, 1 << 29, 1), ((1 << 30) + 1, 1, 1 << 29, 1))]:
        assert want_extent(*accepted) is not None and want_extent(*refused) is None
        assert got_extent(*accepted) == want_extent(*accepted), accepted
        assert got_extent(*refused) is None, refused
        assert b"overflows" in _lib.lib().pmx_last_error()
    assert want_extent(*(3, 2, (LIMIT - 2) // 2, 1 + (LIMIT - 2) % 2)) == LIMIT
    for view in [(SIZE_MAX, SIZE_MAX, SIZE_MAX, SIZE_MAX), (2, 2, SIZE_MAX, SIZE_MAX), (SIZE_MAX, 1, 2, 1), (1 << 32, 1 << 32, 1 << 32, 1 << 32),
                 (3, 3, 1 << 63, 1 << 63)]:                                             # products and sums that wrap 64 bits
        assert want_extent(*view) is None and got_extent(*view) is None, view
    assert _lib.lib().pmx_matrix_view_extent(2, 2, 2, 1, None) == _lib.PMX_ERR_ARG and b"null" in _lib.lib().pmx_last_error()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_refusals_before_a_context_is_read():
    """host arrays stand in for device memory: every call is refused before it reads its context or launches"""
    lib = _lib.lib()
    m = np.zeros((64, 4), dtype=np.uint64)
    out = np.full((64, 4), 0x77, dtype=np.uint64)
    idx = np.zeros(2, dtype=np.uint64)
    ok = np.full(2, 9, dtype=np.uint8)
    fake = _p(m)                                              # never dereferenced
    M, O, I, K = _p(m), _p(out), _p(idx), _p(ok)
    big = 1 << 59
    leaves, commit, opened, verify = lib.pmx_matrix_leaves_dev, lib.pmx_matrix_commit_dev, lib.pmx_matrix_open_dev, lib.pmx_matrix_verify_rows_dev
    cases = [
        (leaves, (None, M, 2, 3, 1, 2, O, None), b"null"),
        (leaves, (fake, None, 2, 3, 1, 2, O, None), b"null"),
        (leaves, (fake, M, 2, 3, 1, 2, None, None), b"null"),
        (leaves, (fake, M, 0, 3, 1, 2, O, None), b"at least one row"),
        (leaves, (fake, M, 2, 0, 1, 2, O, None), b"at least one element"),
        (leaves, (fake, M, 2, 3, 0, 2, O, None), b"stride"),
        (leaves, (fake, M, 2, 3, 1, 0, O, None), b"stride"),
        (leaves, (fake, M, big, 1, 1, 1, O, None), b"overflows"),
        (leaves, (fake, M, 2, 3, 1, big, O, None), b"overflows"),
        (leaves, (fake, M, big - 1, 1, 1, 1, O, None), b"too large"),          # the bytes fit, the launch grid does not
        (commit, (None, M, 2, 3, 1, 2, 2, O, None), b"null"),
        (commit, (fake, None, 2, 3, 1, 2, 2, O, None), b"null"),
        (commit, (fake, M, 2, 3, 1, 2, 2, None, None), b"null"),
        (commit, (fake, M, 0, 3, 1, 2, 2, O, None), b"at least one row"),
        (commit, (fake, M, 2, 3, 0, 2, 2, O, None), b"stride"),
        (commit, (fake, M, 2, big, 1, 2, 2, O, None), b"overflows"),
        (commit, (fake, M, big - 1, 1, 1, 1, 2, O, None), b"too large"),
        (commit, (fake, M, 2, 3, 1, 2, 1, O, None), b"arity"),
        (commit, (fake, M, 2, 3, 1, 2, 0, O, None), b"arity"),
        (opened, (None, M, 2, 3, 1, 2, O, 2, I, 2, O, O, None), b"null"),
        (opened, (fake, None, 2, 3, 1, 2, O, 2, I, 2, O, O, None), b"null"),
        (opened, (fake, M, 2, 3, 1, 2, O, 2, None, 2, O, O, None), b"null"),
        (opened, (fake, M, 2, 3, 1, 2, O, 2, I, 2, None, O, None), b"null"),
        (opened, (fake, M, 2, 3, 1, 2, None, 2, I, 2, O, O, None), b"d_paths without d_nodes"),
        (opened, (fake, M, 0, 3, 1, 2, O, 2, I, 2, O, O, None), b"at least one row"),
        (opened, (fake, M, 2, 0, 1, 2, O, 2, I, 2, O, O, None), b"at least one element"),
        (opened, (fake, M, 2, 3, 1, 0, O, 2, I, 2, O, O, None), b"stride"),
        (opened, (fake, M, 2, 3, big, 2, O, 2, I, 2, O, O, None), b"overflows"),
        (opened, (fake, M, big - 1, 1, 1, 1, None, 2, I, 2, O, None, None), b"too large"),
        (opened, (fake, M, 2, 3, 1, 2, O, 1, I, 2, O, O, None), b"arity"),
        (verify, (None, M, 3, I, O, 1, 2, 2, 2, O, K, O, None), b"null"),
        (verify, (fake, None, 3, I, O, 1, 2, 2, 2, O, K, O, None), b"null"),
        (verify, (fake, M, 3, None, O, 1, 2, 2, 2, O, K, O, None), b"null"),
        (verify, (fake, M, 3, I, None, 1, 2, 2, 2, O, K, O, None), b"null"),
        (verify, (fake, M, 3, I, O, 1, 2, 2, 2, None, K, O, None), b"null"),
        (verify, (fake, M, 3, I, O, 1, 2, 2, 2, O, None, O, None), b"null"),
        (verify, (fake, M, 3, I, O, 1, 2, 2, 2, O, K, None, None), b"null"),
        (verify, (fake, M, 0, I, O, 1, 2, 2, 2, O, K, O, None), b"at least one element"),
        (verify, (fake, M, 3, I, O, 1, 2, 0, 2, O, K, O, None), b"at least one leaf"),
        (verify, (fake, M, 3, I, O, 1, 1, 2, 2, O, K, O, None), b"arity"),
        (verify, (fake, M, 3, I, O, 3, 2, 2, 2, O, K, O, None), b"depth 3 is not the depth 1"),
    ]
    for fn, args, needle in cases:
        assert fn(*args) == _lib.PMX_ERR_ARG, (fn.__name__, args)
        assert needle in lib.pmx_last_error(), (fn.__name__, needle, lib.pmx_last_error())
    assert (out == 0x77).all() and (ok == 9).all() and not m.any(), "a refusal wrote something"
