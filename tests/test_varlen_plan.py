"""Variable-length rows of the absorb driver, on the CPU: the walk of the ragged pass kernels (sponge_amd/csrc/pmx_kernels.hpp:
sponge_walk, sponge_first_kernel, permute_listed_kernel with RowsRagged) restated over one sponge in tests/varlen_plan/varlen_walk.cpp,
on the plan and the ragged-row helpers of pmx_sponge_plan.hpp compiled for the host, with the C oracle's permutation.  For every mode
(tag, index 0..rate) and row length 0..3 rate + 2 at rates 1, 2, 3 and 8 the walk must end with the state and mode words of the
reference's absorb (src/poseidon/mod.rs:232-254, 121-150; oracle/cref's sponge_absorb) - the same elements added, the same
permutations in the same order -, an empty row must touch nothing (:234-236), and a sponge must stop at its own last pass whatever
the call's longest row.  Plus the argument checks of the four entry points that need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sponge_amd as S
from sponge_amd import _lib, synth
from oracle import cref
from oracle import poseidon_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "varlen_plan", "varlen_walk.cpp")
PERMUTE = ctypes.CFUNCTYPE(None, ctypes.c_void_p)


@pytest.fixture(scope="module")
def vw(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("varlen_plan") / "libvarlen_walk.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-DPMX_HOSTCHECK",
                           "-I", os.path.join(ROOT, "sponge_amd", "csrc"), SRC, "-o", out])
    lib = ctypes.CDLL(out)
    lib.vw_absorb.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
                              ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                              PERMUTE, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    lib.vw_row_len.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
    lib.vw_row_len.restype = ctypes.c_uint32
    lib.vw_last_pass.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    lib.vw_last_pass.restype = ctypes.c_uint32
    return lib


def _reference_permutations(tag, index, length, rate):
    """how often the reference's absorb permutes (mod.rs:232-254, 121-150)"""
    if length == 0:
        return 0
    perms, idx = 0, index
    if tag != S.MODE_ABSORBING or index == rate:
        perms, idx = 1, 0
    while idx + length > rate:
        length -= rate - idx
        perms, idx = perms + 1, 0
    return perms


def _walk(vw, cr, rate, state, tag, index, io, lo, hi, max_len):
    t = cr.cfg.t
    trace = []

    def permute(ptr):
        view = np.ctypeslib.as_array((ctypes.c_uint64 * (t * 4)).from_address(ptr))
        trace.append(view.copy())
        view[:] = cr.permute_batch(view.reshape(1, t, 4)).reshape(-1)

    p32 = np.frombuffer(np.array(O.to_limbs(cr.cfg.p), dtype=np.uint64).tobytes(), dtype=np.uint32).copy()
    st = np.ascontiguousarray(state, dtype=np.uint64).copy()
    tg, ix = ctypes.c_uint32(tag), ctypes.c_uint32(index)
    perms, steps = ctypes.c_uint32(), ctypes.c_uint32()
    cb = PERMUTE(permute)
    rc = vw.vw_absorb(rate, cr.cfg.capacity, p32.ctypes.data, st.ctypes.data, ctypes.byref(tg), ctypes.byref(ix), io.ctypes.data,
                      lo, hi, max_len, cb, ctypes.byref(perms), ctypes.byref(steps))
    assert perms.value == len(trace)
    return rc, st, tg.value, ix.value, trace, steps.value


@pytest.mark.parametrize("rate", [1, 2, 3, 8])
def test_ragged_walk_equals_the_reference_absorb(vw, rate):
    f = S.BLS12_381_FR
    cr = cref.CRef(O.make_config(O.BLS12_381_FR, 255, rate, 5, 8, 31))
    t = rate + 1
    longest = 3 * rate + 2
    io = synth.random_elements(f, longest + 8, seed=0xA0 + rate)
    checked = 0
    for tag in (S.MODE_ABSORBING, S.MODE_SQUEEZING):
        for index in range(rate + 1):
            state = synth.random_elements(f, t, seed=1000 * rate + 10 * index + tag)
            for length in range(longest + 1):
                lo = 5
                row = io[lo:lo + length]
                want_state, want_tag, want_index = cr.sponge_absorb(state, tag, index, row)
                # the row alone in its call (max_len = its length), and among longer rows (the call's bound, and a bound far beyond:
                # the sponge must stop at its own last pass, in the same number of steps)
                runs = [_walk(vw, cr, rate, state, tag, index, io, lo, lo + length, m) for m in (length, longest, 65536 * rate)]
                for rc, st, tg, ix, trace, steps in runs:
                    assert rc == 0, (rate, tag, index, length, rc)
                    if length == 0:   # untouched: nothing read, nothing written, mode words as they were (mod.rs:234-236)
                        assert not trace and steps == 0 and np.array_equal(st, state) and (tg, ix) == (tag, index)
                        continue
                    assert np.array_equal(st, want_state), (rate, tag, index, length)
                    assert (tg, ix) == (want_tag, want_index), (rate, tag, index, length, tg, ix, want_tag, want_index)
                    assert len(trace) == _reference_permutations(tag, index, length, rate), (rate, tag, index, length)
                    assert steps <= vw.vw_last_pass(length, rate) + 1, (rate, tag, index, length, steps)
                # the same data in the same order: every state the permutation was handed is the same in the three calls
                for _, _, _, _, trace, steps in runs[1:]:
                    assert len(trace) == len(runs[0][4]) and all(np.array_equal(a, b) for a, b in zip(trace, runs[0][4]))
                    assert steps == runs[0][5]
                checked += 1
    assert checked == 2 * (rate + 1) * (longest + 1)


def test_ragged_rows_clamp_and_decreasing_offsets(vw):
    """the device reads what it is given: a decreasing pair is an empty row, a row longer than max_len is absorbed up to max_len"""
    assert vw.vw_row_len(7, 3, 100) == 0 and vw.vw_row_len(3, 3, 100) == 0
    assert vw.vw_row_len(3, 10, 100) == 7 and vw.vw_row_len(3, 1000, 100) == 100 and vw.vw_row_len(0, 1 << 40, 5) == 5
    rate = 3
    f = S.BLS12_381_FR
    cr = cref.CRef(O.make_config(O.BLS12_381_FR, 255, rate, 5, 8, 31))
    io = synth.random_elements(f, 40, seed=77)
    state = synth.random_elements(f, rate + 1, seed=78)
    rc, st, tg, ix, trace, _ = _walk(vw, cr, rate, state, S.MODE_SQUEEZING, rate, io, 9, 4, 8)
    assert rc == 0 and not trace and np.array_equal(st, state) and (tg, ix) == (S.MODE_SQUEEZING, rate)
    rc, st, tg, ix, _, _ = _walk(vw, cr, rate, state, S.MODE_ABSORBING, 1, io, 2, 30, 8)
    want = cr.sponge_absorb(state, S.MODE_ABSORBING, 1, io[2:10])
    assert rc == 0 and np.array_equal(st, want[0]) and (tg, ix) == (want[1], want[2])


def test_varlen_entries_reject_bad_arguments_without_a_device():
    """null ctx, and null offsets with n > 0, are PMX_ERR_ARG before the context is read or a device is touched"""
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.uint64)
    tag = np.zeros(2, dtype=np.uint32)
    off = np.array([0, 1, 2], dtype=np.uint64)
    p = buf.ctypes.data
    assert lib.pmx_hash_varlen_batch(None, p, off.ctypes.data, p, 1, 2) == _lib.PMX_ERR_ARG
    assert lib.pmx_hash_varlen_batch_dev(None, p, off.ctypes.data, 1, p, 1, 2, None) == _lib.PMX_ERR_ARG
    assert lib.pmx_sponge_absorb_varlen_batch(None, p, tag.ctypes.data, tag.ctypes.data, p, off.ctypes.data, 2) == _lib.PMX_ERR_ARG
    assert lib.pmx_sponge_absorb_varlen_batch_dev(None, p, tag.ctypes.data, tag.ctypes.data, p, off.ctypes.data, 1, 2, None) == _lib.PMX_ERR_ARG
    # a context handle that is never dereferenced: the argument checks come first
    fake = ctypes.c_void_p(buf.ctypes.data)
    assert lib.pmx_hash_varlen_batch(fake, p, None, p, 1, 2) == _lib.PMX_ERR_ARG
    assert b"null" in lib.pmx_last_error()
    assert lib.pmx_hash_varlen_batch_dev(fake, p, None, 1, p, 1, 2, None) == _lib.PMX_ERR_ARG
    assert lib.pmx_sponge_absorb_varlen_batch(fake, p, tag.ctypes.data, tag.ctypes.data, p, None, 2) == _lib.PMX_ERR_ARG
    assert lib.pmx_sponge_absorb_varlen_batch_dev(fake, p, tag.ctypes.data, tag.ctypes.data, p, None, 1, 2, None) == _lib.PMX_ERR_ARG
