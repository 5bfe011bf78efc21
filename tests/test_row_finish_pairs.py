"""The paired row finish of the matrix-core layers (sponge_amd/csrc/pmx_mfma.hpp: mfma_pair_sums, mfma_row_acc_pairs_p) on the CPU.

A row of at most 15 inputs folds its 32 byte sums in pairs, Q = S_e + 256 S_{e+1}, before they change lanes, and a word of the row is
corr + carry + Q0 + Q1 2^16 + m p_w.  The host build returns the nine words a[] of V + m p from that form and from the four-weight form
(mfma_row_acc_p), which rows of 16 inputs and more keep; both must be the same words, and the words Python's integers give.  The sums go
to the ends of what a row of NIN inputs can hold, |S_e| <= 32 NIN 2^14, with the signs arranged so that a pair's borrow and a word's carry
are at their worst.  Then whole permutations through the host templates, where every pair of every row is checked to fit 32 bits."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from sponge_amd._lib import PmxConfig
from oracle import cref
from oracle import poseidon_oracle as O

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")
CSRC = os.path.join(os.path.dirname(HERE), os.pardir, "sponge_amd", "csrc")
P25519 = (1 << 255) - 19
MODULI = [O.BLS12_381_FR, O.BN254_FR, P25519]
PAIRED_INPUTS = [3, 5, 9, 15]


@pytest.fixture(scope="module")
def hc():
    # pmx_row_finish_check.cpp: pmx_hostcheck.cpp's templates and entries plus the guard on the pairs and the row finish row by row
    so = os.path.join(HERE, "libpmx_row_finish_check.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC,
                           os.path.join(HERE, "pmx_row_finish_check.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.hc_row_finish.argtypes = [ctypes.c_void_p] * 6
    lib.hc_row_form.argtypes = [ctypes.c_int]
    lib.hc_permute_hybrid_mfma.argtypes = [ctypes.POINTER(PmxConfig), ctypes.c_void_p, ctypes.c_size_t]
    return lib


def row_finish(hc, p, sums, corr):
    mod = np.array(O.to_limbs(p), dtype=np.uint64)
    s = np.array(sums, dtype=np.int32)
    c = np.array(corr, dtype=np.int64)
    a_pairs, a_four, limbs = (np.zeros(9, dtype=np.uint32) for _ in range(3))
    assert hc.hc_row_finish(mod.ctypes.data, s.ctypes.data, c.ctypes.data, a_pairs.ctypes.data, a_four.ctypes.data, limbs.ctypes.data) == 0
    return [int(x) for x in a_pairs], [int(x) for x in a_four], [int(x) for x in limbs]


def expected(p, sums, corr):
    """the words of V + m p and the limbs of (V + m p) >> 24 from Python integers"""
    v = sum(s << (8 * e) for e, s in enumerate(sums)) + sum(c << (32 * w) for w, c in enumerate(corr))
    m = (v * (-pow(p, -1, 1 << 24))) % (1 << 24)
    total = v + m * p
    assert total >= 0 and total % (1 << 24) == 0 and total >> 256 < (1 << 31)
    words = [(total >> (32 * w)) & 0xFFFFFFFF for w in range(8)] + [total >> 256]
    row = total >> 24
    limbs = [(row >> (29 * k)) & ((1 << 29) - 1) for k in range(8)] + [row >> 232]
    return words, limbs


def offset_corr(big):
    """correction words that lift every sum by `big` - V is not negative whatever the signs of the sums, as for a real row (V = sum u Y)"""
    return [big * 0x01010101] * 8


def sign_patterns(big):
    yield "all +", [big] * 32
    yield "all -", [-big] * 32
    yield "+ - within a pair", [big if e % 2 == 0 else -big for e in range(32)]
    yield "- + within a pair", [-big if e % 2 == 0 else big for e in range(32)]
    yield "+ + - - across the pairs of a word", [big if e % 4 < 2 else -big for e in range(32)]
    yield "- - + + across the pairs of a word", [-big if e % 4 < 2 else big for e in range(32)]
    yield "+ - - + ", [big if e % 4 in (0, 3) else -big for e in range(32)]
    yield "words alternate", [big if (e // 4) % 2 == 0 else -big for e in range(32)]
    yield "one short of the bound, alternating", [(big - 1) if e % 2 else -(big - 1) for e in range(32)]
    yield "zero", [0] * 32


@pytest.mark.parametrize("p", MODULI)
@pytest.mark.parametrize("n_in", PAIRED_INPUTS)
def test_sums_at_the_ends_of_their_range(hc, p, n_in):
    big = 32 * n_in * (1 << 14)
    assert 257 * big < (1 << 31)
    for what, sums in sign_patterns(big):
        for corr in (offset_corr(big), [c + (7 << 33) for c in offset_corr(big)]):
            a_pairs, a_four, limbs = row_finish(hc, p, sums, corr)
            words, want_limbs = expected(p, sums, corr)
            assert a_pairs == a_four, (what, n_in)
            assert a_pairs == words, (what, n_in)
            assert limbs == want_limbs, (what, n_in)


@pytest.mark.parametrize("p", MODULI)
@pytest.mark.parametrize("n_in", PAIRED_INPUTS)
def test_random_rows(hc, p, n_in):
    rng = random.Random(1000 * n_in + p % 997)
    big = 32 * n_in * (1 << 14)
    seen0, bad0 = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    hc.hc_row_pairs(ctypes.byref(seen0), ctypes.byref(bad0))
    for i in range(300):
        sums = [rng.choice((-big, big, rng.randint(-big, big), rng.randint(-300, 300))) for _ in range(32)]
        corr = [c + rng.randrange(1 << 40) for c in offset_corr(big)]
        a_pairs, a_four, limbs = row_finish(hc, p, sums, corr)
        words, want_limbs = expected(p, sums, corr)
        assert a_pairs == a_four == words, (n_in, i)
        assert limbs == want_limbs, (n_in, i)
    seen, too_large = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    hc.hc_row_pairs(ctypes.byref(seen), ctypes.byref(too_large))
    assert seen.value - seen0.value == 300 * 16 and too_large.value == bad0.value


def test_rows_of_16_inputs_and_more_keep_the_four_weight_form(hc):
    """the compile-time predicate, asked through the templates' own dispatch (mfma_row_acc_for): pairs up to 15 inputs, not at 16 (the bound
    257 * 32 * 16 * 2^14 = 2 155 872 256 is past 2^31) nor at 17, the window layers of t = 9"""
    assert 257 * 32 * 15 * (1 << 14) == 2021130240 < (1 << 31) <= 2155872256 == 257 * 32 * 16 * (1 << 14)
    for n_in in PAIRED_INPUTS + [1, 2, 4, 8, 13]:
        assert hc.hc_row_form(n_in) == 1, n_in
    for n_in in (16, 17, 18, 33):
        assert hc.hc_row_form(n_in) == 0, n_in


def test_a_pair_past_the_bound_is_counted(hc):
    """the guard itself: sums a row of 16 inputs could hold make a pair that does not fit, and the host build says so"""
    seen0, bad0 = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    hc.hc_row_pairs(ctypes.byref(seen0), ctypes.byref(bad0))
    big = 32 * 16 * (1 << 14)
    row_finish(hc, O.BLS12_381_FR, [big] * 32, offset_corr(big))
    seen, bad = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    hc.hc_row_pairs(ctypes.byref(seen), ctypes.byref(bad))
    assert seen.value == seen0.value + 16 and bad.value == bad0.value + 16


def _states(p, t, seed):
    rng = random.Random(seed)
    pat7f = int.from_bytes(b"\x7f" * 32, "little") % p
    pat80 = int.from_bytes(b"\x80" * 32, "little") % p
    mixed = int.from_bytes(b"\x7f\x80" * 16, "little") % p
    rows = [[rng.randrange(p) for _ in range(t)] for _ in range(12)]
    rows += [[0] * t, [p - 1] * t, [pat7f] * t, [pat80] * t, [mixed] * t, [pat7f, pat80] * (t // 2) + [mixed] * (t % 2)]
    return cref.elems_to_limbs([x for r in rows for x in r], p).reshape(len(rows), t, 4)


@pytest.mark.parametrize("p,bits,t,rp", [(O.BLS12_381_FR, 255, 3, 31), (O.BN254_FR, 254, 3, 57), (O.BLS12_381_FR, 255, 4, 56),
                                         (O.BLS12_381_FR, 255, 8, 57), (O.BN254_FR, 254, 9, 57), (O.BLS12_381_FR, 255, 9, 57)])
def test_whole_permutations_through_the_host_templates(hc, p, bits, t, rp):
    """every layer and history row of the window engines through the paired finish where its input count allows (t = 9: paired dense and
    history rows beside unpaired window rows), against the C restatement; every pair formed on the way fits 32 bits"""
    cfg = O.make_config(p, bits, t - 1, 5, 8, rp)
    states = _states(p, t, 31 * t + rp)
    want = cref.CRef(cfg).permute_batch(states, threads=0)
    ark = cref.elems_to_limbs([v for row in cfg.ark for v in row], p)
    mds = cref.elems_to_limbs([v for row in cfg.mds for v in row], p)
    c = PmxConfig()
    c.full_rounds, c.partial_rounds, c.alpha, c.rate, c.capacity = 8, rp, 5, t - 1, 1
    for i, l in enumerate(O.to_limbs(p)):
        c.modulus[i] = l
    c.ark, c.mds = ark.ctypes.data, mds.ctypes.data
    seen0, bad0 = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    hc.hc_row_pairs(ctypes.byref(seen0), ctypes.byref(bad0))
    out = states.copy()
    assert hc.hc_permute_hybrid_mfma(ctypes.byref(c), out.ctypes.data, len(states)) == 0
    assert np.array_equal(out, want)
    seen, bad = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    hc.hc_row_pairs(ctypes.byref(seen), ctypes.byref(bad))
    # 16 pairs a row; at least the 8 dense layers' t rows took the paired form
    assert seen.value - seen0.value >= 16 * 8 * t * len(states) and bad.value == bad0.value
    ins, too_large = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    hc.hc_layer_inputs(ctypes.byref(ins), ctypes.byref(too_large))
    assert ins.value > 0 and too_large.value == 0
