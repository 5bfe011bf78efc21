"""The memory footprint of pmx_merkle_ary_update_dev, as tests/test_gpu_merkle_ary_footprint.py does it for the other *_dev entries of
the arity-k trees: all buffers of the call carved out of ONE poisoned device allocation at the documented alignment and nothing above it
(d_nodes, d_new_leaves and d_work at 16 bytes, d_indices at 8), 256 KiB of guard around each (tests/arena.py).  After the call the node
array equals the C port's rebuild in full - so only the leaf rows and the ancestors changed in it -, the two input buffers are as they
were, and every byte outside the four buffers is unchanged.

One window-engine case (BN254 t = 9, arity 8, 4096 leaves) and one run-time-width case (t = 16, arity 15, 3375 leaves), k = 65 - one full
wave and one lane: the first level runs as gathered rows (65 < 512, 65 < 225 parents), the levels above as whole levels.  Each case runs
with in-range indices and again with indices that name no leaf mixed in, and once more on the control layout (every buffer at a multiple
of 256 bytes)."""
import numpy as np
import pytest
import torch

from sponge_amd import _lib, synth

import arena
import merkle_ary_oracle as M
from test_gpu_footprint import DeviceArena

pytestmark = pytest.mark.gpu

E = arena.E
CASES = [("t9-bn254", 8, 4096), ("lds-t16", 15, 3375)]
UNITS = 65
U64 = (1 << 64) - 1


def update_buffers(n_nodes, a, k):
    return [("d_nodes", n_nodes * E, 16, "inout"), ("d_indices", k * 8, 8, "in"), ("d_new_leaves", k * E, 16, "in"),
            ("d_work", k * (a + 1) * 4 * 8, 16, "scratch")]


def _case(label, a, m, out_of_range):
    """(indices, new leaves, the oracle's old tree, its rebuild with the in-range updates applied)"""
    f, cfg, cr = M.config(label)
    leaves, old = M.cached_tree(label, a, m)
    idx = M.path_indices(m, a, UNITS, seed=a + 1)
    idx = np.array(list(dict.fromkeys(int(x) for x in idx)), dtype=np.uint64)      # distinct
    rng = np.random.default_rng(a)
    while len(idx) < UNITS:
        extra = np.uint64(rng.integers(0, m))
        if extra not in idx:
            idx = np.append(idx, extra)
    new = synth.random_elements(f, UNITS, seed=600 + a)
    if out_of_range:
        idx[3], idx[17], idx[64] = m, U64, m + 7
    after = np.array(leaves, dtype=np.uint64)
    for i, j in enumerate(int(x) for x in idx):
        if j < m:
            after[j] = new[i]
    return idx, new, old, M.tree(cr, after, a)


@pytest.mark.parametrize("out_of_range", [False, True])
@pytest.mark.parametrize("label,a,m", CASES)
def test_merkle_ary_update_dev(label, a, m, out_of_range):
    idx, new, old, want = _case(label, a, m, out_of_range)
    assert m // a > UNITS >= m // (a * a), "gathered rows at the first level, whole levels above"
    h = M.config(label)[1].context()._h
    for control in (False, True):
        ar = DeviceArena(update_buffers(old.shape[0], a, UNITS), seed=11, control=control)
        ar.put("d_nodes", old)
        ar.put("d_indices", idx)
        ar.put("d_new_leaves", new)
        ar.upload()
        if not control:
            assert ar.ptr("d_indices") % 16 == 8
        _lib.check(_lib.lib().pmx_merkle_ary_update_dev(h, ar.ptr("d_nodes"), m, a, ar.ptr("d_indices"), ar.ptr("d_new_leaves"), UNITS,
                                                        ar.ptr("d_work"), torch.cuda.current_stream().cuda_stream))
        ar.finish()
        assert np.array_equal(ar.get("d_nodes").reshape(-1, 4), want), (label, control, out_of_range)


@pytest.mark.parametrize("label,a,m", CASES)
def test_an_element_pointer_at_8_mod_16_is_refused(label, a, m):
    idx, new, old, want = _case(label, a, m, False)
    L, h, s = _lib.lib(), M.config(label)[1].context()._h, torch.cuda.current_stream().cuda_stream
    ar = DeviceArena(update_buffers(old.shape[0], a, UNITS), seed=12)
    ar.put("d_nodes", old)
    ar.put("d_indices", idx)
    ar.put("d_new_leaves", new)
    ar.upload()
    for name in ("d_nodes", "d_new_leaves", "d_work"):
        p = {n: ar.ptr(n, 8 if n == name else 0) for n in ("d_nodes", "d_indices", "d_new_leaves", "d_work")}
        rc = L.pmx_merkle_ary_update_dev(h, p["d_nodes"], m, a, p["d_indices"], p["d_new_leaves"], UNITS, p["d_work"], s)
        assert rc == _lib.PMX_ERR_ARG and b"16-byte aligned" in L.pmx_last_error(), (name, L.pmx_last_error())
        ar.unchanged()
