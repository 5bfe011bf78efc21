"""How the host-buffer sponge entries cut a call that is longer than one device call may be (sponge_amd/csrc/pmx_host_pieces.hpp; the
entries are sponge_host, squeeze_cut_host and varlen_host of pmx_sponge.cpp), on the CPU: the header compiled for the host behind
tests/host_pieces/pieces_host.cpp, with max_len shrunk to a few rates.
- The cut of a fixed-length call: positive pieces of at most max_len that sum to the call, none but the first exactly one rate.
- The same cut against the C oracle (oracle/cref: sponge_squeeze, sponge_absorb): piece by piece is one whole call - outputs, end state
  and mode words - in every mode; and the cut WITHOUT the rule (plain min) is not, exactly where a last piece of one rate meets a
  sponge that squeezes from inside its rate (the test of src/poseidon/mod.rs:175 skips a permutation the long call performs).
- The ragged cut of the variable-length absorb: the pieces tile every row in order and the rebased offsets are their running sums.
- tests/host_pieces/sanitize_main.cpp, a program of its own, walks the same ranges under ASan + UBSan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sponge_amd as S
from sponge_amd import synth
from oracle import cref
from oracle import poseidon_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sponge_amd", "csrc")
HERE = os.path.join(ROOT, "tests", "host_pieces")
MAX_RATES = (3, 4, 7)


@pytest.fixture(scope="module")
def hp(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_pieces") / "libpieces_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-DPMX_HOSTCHECK", "-I", CSRC,
                           os.path.join(HERE, "pieces_host.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    z = ctypes.c_size_t
    lib.hp_max_passes.restype = z
    lib.hp_fixed_piece.argtypes, lib.hp_fixed_piece.restype = [z, z, z, z], z
    lib.hp_ragged_pieces.argtypes, lib.hp_ragged_pieces.restype = [z, z], z
    lib.hp_ragged_range.argtypes, lib.hp_ragged_range.restype = [z, z, z, ctypes.POINTER(z), ctypes.POINTER(z)], None
    lib.hp_ragged_offsets.argtypes, lib.hp_ragged_offsets.restype = [ctypes.c_void_p, z, z, z, ctypes.c_void_p], None
    return lib


def _cut(hp, total, max_len, rate):
    """the pieces of the walk every host entry runs: do { piece } while (done < total)"""
    pieces, done = [], 0
    while True:
        pieces.append(hp.hp_fixed_piece(done, total, max_len, rate))
        done += pieces[-1]
        if done >= total:
            return pieces


def _plain_cut(total, max_len):
    pieces, done = [], 0
    while True:
        pieces.append(min(total - done, max_len))
        done += pieces[-1]
        if done >= total:
            return pieces


def _totals(max_len, rate):
    return range(3 * max_len + 2 * rate + 1)


@pytest.mark.parametrize("rate", [1, 2, 3, 8])
def test_fixed_cut_sums_to_the_call_and_only_the_first_piece_may_be_one_rate(hp, rate):
    assert hp.hp_max_passes() == 65536
    for k in MAX_RATES:
        max_len = k * rate
        for total in _totals(max_len, rate):
            pieces = _cut(hp, total, max_len, rate)
            assert sum(pieces) == total, (rate, max_len, total, pieces)
            assert all(0 < p <= max_len for p in pieces) or pieces == [0], (rate, max_len, total, pieces)
            assert rate not in pieces[1:], (rate, max_len, total, pieces)
            if total <= max_len:
                assert pieces == [total]          # a call within the limit is the walk with one piece: the caller's own call
            if total % max_len != rate or total <= max_len:
                assert pieces == _plain_cut(total, max_len)   # the rule changes a cut only where it is needed


@pytest.mark.parametrize("rate", [1, 2, 3])
def test_fixed_cut_piece_by_piece_is_one_whole_call_to_the_c_oracle(hp, rate):
    f = S.BLS12_381_FR
    cr = cref.CRef(O.make_config(O.BLS12_381_FR, 255, rate, 5, 8, 31))
    t = rate + 1
    longest = 3 * max(MAX_RATES) * rate + 2 * rate
    elems = synth.random_elements(f, longest, seed=0xC0 + rate)

    def squeeze(sponge, pieces):
        outs = []
        for p in pieces:
            *sponge, o = cr.sponge_squeeze(*sponge, p)
            outs.append(o)
        return np.concatenate(outs), sponge

    def absorb(sponge, pieces):
        done = 0
        for p in pieces:
            if p:                                 # absorbing nothing is not a call (mod.rs:234-236)
                sponge = cr.sponge_absorb(*sponge, elems[done:done + p])
            done += p
        return sponge

    def same(a, b):
        return np.array_equal(a[0], b[0]) and tuple(a[1:]) == tuple(b[1:])

    plain_differs = set()
    for tag in (S.MODE_ABSORBING, S.MODE_SQUEEZING):
        for index in range(rate + 1):
            start = (synth.random_elements(f, t, seed=1000 * rate + 10 * index + tag), tag, index)
            whole = {}
            for k in MAX_RATES:
                max_len = k * rate
                for total in _totals(max_len, rate):
                    if total not in whole:
                        whole[total] = (squeeze(start, [total]), absorb(start, [total]))
                    (want_out, want_sq), want_ab = whole[total]
                    pieces = _cut(hp, total, max_len, rate)
                    out, sponge = squeeze(start, pieces)
                    assert np.array_equal(out, want_out) and same(sponge, want_sq), ("squeeze", rate, tag, index, max_len, total, pieces)
                    assert same(absorb(start, pieces), want_ab), ("absorb", rate, tag, index, max_len, total, pieces)
                    plain = _plain_cut(total, max_len)
                    if plain != pieces:
                        out, sponge = squeeze(start, plain)
                        if not (np.array_equal(out, want_out) and same(sponge, want_sq)):
                            plain_differs.add((tag, index, max_len, total))
                        assert same(absorb(start, plain), want_ab)   # absorbing needs no rule
    # Without the rule the last piece is exactly one rate wherever total = j max_len + rate: to a sponge that stands inside its rate
    # (Squeezing{i}, 0 < i < rate; a piece of whole rates leaves it there) that call is not the tail of the long one.  At index 0 or
    # rate, and from Absorbing (which ends the first piece at Squeezing{rate}), the piece starts on a rate boundary and is harmless.
    want_differs = {(S.MODE_SQUEEZING, index, k * rate, j * k * rate + rate)
                    for index in range(1, rate) for k in MAX_RATES for j in (1, 2, 3) if j * k * rate + rate in _totals(k * rate, rate)}
    assert plain_differs == want_differs
    assert (rate == 1) == (not plain_differs)     # rate 1 has no inside; at rates 2 and 3 this test can fail


@pytest.mark.parametrize("piece", [1, 2, 5])
def test_ragged_cut_tiles_every_row_and_rebases_the_offsets(hp, piece):
    z = ctypes.c_size_t
    for longest in range(4 * piece + 3):
        lengths = list(range(longest + 1)) + [longest, 0, longest // 2]      # every length up to the longest, in one call
        offsets = np.cumsum([7] + lengths).astype(np.uint64)                  # the caller's offsets need not start at 0
        n = len(lengths)
        pieces = hp.hp_ragged_pieces(longest, piece)
        assert pieces == -(-longest // piece)
        cursor = [0] * n
        for k in range(pieces):
            off = np.full(n + 1, 0xFFFF, dtype=np.uint64)
            hp.hp_ragged_offsets(offsets.ctypes.data, n, piece, k, off.ctypes.data)
            widths = []
            for i, length in enumerate(lengths):
                lo, hi = z(), z()
                hp.hp_ragged_range(length, piece, k, ctypes.byref(lo), ctypes.byref(hi))
                assert lo.value == cursor[i] and lo.value <= hi.value <= length and hi.value - lo.value <= piece, (piece, longest, k, i)
                assert (lo.value, hi.value) == (min(length, k * piece), min(length, (k + 1) * piece))   # the boundaries varlen_host has always had
                cursor[i] = hi.value
                widths.append(hi.value - lo.value)
            assert [int(x) for x in off] == [int(x) for x in np.cumsum([0] + widths)], (piece, longest, k)
            if pieces == 1:
                assert np.array_equal(off, offsets - offsets[0])
        assert cursor == lengths, (piece, longest)


# ---- the header under the sanitizers: a program of its own, nothing sanitized is loaded into this process ----------------------------
def test_host_pieces_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "host_pieces_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-DPMX_HOSTCHECK", "-I", CSRC, os.path.join(HERE, "sanitize_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "sanitized ok" in out.stdout, out.stdout + out.stderr
