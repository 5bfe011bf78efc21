"""The pieces of prepare() (sponge_amd/csrc/pmx_prepare.hpp) that can be checked on their own, through tests/hostcheck: the bytes a residue
is stored as in an int8 table (stored_bytes - its failure used to abort the process, now it is a return value), and the layout of the
table against the section sizes pmx_mfma.hpp states."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from sponge_amd._lib import PmxConfig
from oracle import cref
from oracle import poseidon_oracle as O

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")
P25519 = (1 << 255) - 19
P127 = 0x7FE25EA8BD7912EFEE60F553B2B761E3748A7D8348CBC9AB8D8E5A91E0000001      # top byte 127 (tests/test_p1_step.py)
S = ((1 << 256) - 1) // 255                                                       # 32 balanced bytes reach -128 S .. 127 S
PLAIN, MINUS_P, BROKEN = 0, 1, 2


@pytest.fixture(scope="module")
def hc():
    subprocess.check_call(["make", "-C", HERE, "all"], stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.environ.get("PMX_HOSTCHECK_LIB") or os.path.join(HERE, "libpmx_hostcheck.so"))
    lib.hc_stored_bytes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.hc_layout.argtypes = [ctypes.POINTER(PmxConfig), ctypes.c_void_p]
    return lib


def stored(hc, p, y):
    mod, val = np.array(O.to_limbs(p), dtype=np.uint64), np.array(O.to_limbs(y), dtype=np.uint64)
    out = np.full(32, 99, dtype=np.int8)
    how = hc.hc_stored_bytes(mod.ctypes.data, val.ctypes.data, out.ctypes.data)
    return how, [int(d) for d in out]


@pytest.mark.parametrize("p", [O.BLS12_381_FR, P25519, P127])
def test_balanced_bytes_of_a_residue(hc, p):
    """Every residue has 32 digits in [-128, 127] whose value is Y itself up to 127 S and Y - p above (only a modulus above 127 S has
    such residues); what is no residue - p itself, which the abort used to guard - comes back as a broken invariant."""
    assert (P25519 - 1 > 127 * S) and (O.BLS12_381_FR < 127 * S)         # the list reaches both forms
    for y in [0, 1, 127, 128, 127 * S, 127 * S + 1, p - 1, p]:
        how, d = stored(hc, p, y)
        want = BROKEN if y >= p else MINUS_P if y > 127 * S else PLAIN
        assert how == want, (hex(p), hex(y), how)
        if how == BROKEN:
            continue
        assert all(-128 <= e <= 127 for e in d)
        assert sum(e << (8 * i) for i, e in enumerate(d)) == (y - p if how == MINUS_P else y), (hex(p), hex(y))
    assert stored(hc, p, p)[0] == BROKEN


@pytest.mark.parametrize("t,rp", [(2, 24), (3, 31), (4, 24), (9, 24), (16, 24), (3, 0)])
def test_layout_of_the_table(hc, t, rp):
    """The offsets in the order of the layout comment (Prepared), the int8 sections 16-byte aligned and as long as pmx_mfma.hpp says (the
    export computes that from the header's own functions), the io block last."""
    p, rf = O.BLS12_381_FR, 8
    cfg = O.make_config(p, 255, t - 1, 5, rf, rp)
    ark = cref.elems_to_limbs([v for row in cfg.ark for v in row], p)
    mds = cref.elems_to_limbs([v for row in cfg.mds for v in row], p)
    c = PmxConfig()
    c.full_rounds, c.partial_rounds, c.alpha, c.rate, c.capacity = rf, rp, 5, t - 1, 1
    for i, l in enumerate(O.to_limbs(p)):
        c.modulus[i] = l
    c.ark, c.mds = ark.ctypes.data, mds.ctypes.data
    out = np.zeros(13, dtype=np.uint64)
    assert hc.hc_layout(ctypes.byref(c), out.ctypes.data) == 0
    mds_o, opt_o, coop_o, mfma_o, win_o, io_o, size, has_opt, dense, window, dense_words, window_words, io_words = (int(x) for x in out)
    offsets = [0, mds_o, opt_o, coop_o, mfma_o, win_o, io_o, size]
    assert offsets == sorted(offsets), offsets
    assert mfma_o % 4 == 0
    assert has_opt == (1 if rp else 0) and dense == (1 if rp and 3 <= t <= 9 else 0), (has_opt, dense)
    if dense:
        assert dense_words > 0 and win_o - mfma_o == dense_words
    else:
        assert win_o == mfma_o
    if window:
        assert window_words > 0 and io_o - win_o == window_words
    else:
        assert io_o == win_o
    assert io_o + io_words == size
