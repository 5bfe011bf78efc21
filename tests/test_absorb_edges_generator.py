"""The edge-input generator of the GPU absorb tests (tests/absorb_edges.py) checked on its own, without a GPU: every target
is hit for every config, its lockstep sponges are the C port's sponges, and the raw sums it meant to produce are the raw
sums the pure-Python oracle (pinned by the reference's KATs) sees."""
import random

import numpy as np
import pytest

from oracle import cref
from oracle import poseidon_oracle as O

import absorb_edges as E

PALLAS = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001
P25519 = (1 << 255) - 19
# (id, modulus, prime bits, rate, alpha, RF, RP): the moduli and widths of tests/test_gpu_absorb_edges.py
CONFIGS = [
    ("bls-t3-a5", O.BLS12_381_FR, 255, 2, 5, 8, 31),
    ("bls-t3-a17", O.BLS12_381_FR, 255, 2, 17, 8, 31),
    ("bn254-t3-a5", O.BN254_FR, 254, 2, 5, 8, 57),
    ("pallas-t3-a5", PALLAS, 255, 2, 5, 8, 56),
    ("p25519-t3-a5", P25519, 255, 2, 5, 8, 56),
    ("bls-t2-a5", O.BLS12_381_FR, 255, 1, 5, 8, 31),
    ("bn254-t9-a5", O.BN254_FR, 254, 8, 5, 8, 57),
]


def script_for(rate):
    """the call lengths of the GPU tests: calls that end with and without a permutation after their last addition"""
    ops = [("absorb", 1), ("absorb", rate), ("squeeze", 1), ("absorb", rate + 1), ("absorb", 2 * rate + 2), ("squeeze", rate),
           ("absorb", 10 * rate + 1), ("squeeze", 2 * rate + 1)]
    if rate > 1:
        ops.insert(1, ("absorb", rate - 1))
    return ops


@pytest.mark.parametrize("case", CONFIGS, ids=lambda c: c[0])
def test_generator_hits_every_target_and_tracks_the_c_port(case):
    _, p, bits, rate, alpha, rf, rp = case
    ocfg = O.make_config(p, bits, rate, alpha, rf, rp)
    cr = cref.CRef(ocfg)
    n, t = 64, rate + 1
    st0 = E.edge_states(p, n, t, seed=rate)
    tag0, idx0 = E.mixed_modes(n, rate, seed=rate)
    g = E.EdgeSponges(ocfg, st0, tag0, idx0, seed=3, c_port=cr)
    ref = [(st0[i].copy(), int(tag0[i]), int(idx0[i])) for i in range(n)]
    script = script_for(rate)
    elems_by_call = []
    for op, length in script:
        if op == "absorb":
            elems = g.absorb(length)
            elems_by_call.append(elems)
            ref = [cr.sponge_absorb(s, m, i, elems[j]) for j, (s, m, i) in enumerate(ref)]
        else:
            out = g.squeeze(length)
            elems_by_call.append(None)
            nxt = []
            for j, (s, m, i) in enumerate(ref):
                s2, m2, i2, o = cr.sponge_squeeze(s, m, i, length)
                assert np.array_equal(out[j], o), (op, length, j)
                nxt.append((s2, m2, i2))
            ref = nxt
        assert np.array_equal(g.state, np.stack([s for s, _, _ in ref])), (op, length)
        assert [int(x) for x in g.tag] == [m for _, m, _ in ref] and [int(x) for x in g.idx] == [i for _, _, i in ref], (op, length)
    assert all(g.hits[k] > 0 for k in E.ALL_HITS), g.hits
    # every element is a reduced residue, and the sums the generator recorded are the sums it aimed at
    for c, i, j, s, x, target in g.adds:
        assert 0 <= s < p and 0 <= x < p
        want = {"sum_p": p, "sum_pm1": p - 1, "sum_pp1": p + 1}.get(target)
        if want is not None:
            assert s + x == want
    # a sample of the raw sums recomputed with the pure-Python oracle, its own sponge from the same start
    rng = random.Random(rate * 7 + alpha)
    for i in rng.sample(range(n), 2):
        picks = {}
        for c, ii, j, s, x, target in g.adds:
            if ii == i:
                picks[(c, j)] = (s + x, target)
        chosen = rng.sample(sorted(picks), min(12, len(picks)))
        for target in E.TARGETS:                               # at least one addition of each target this sponge met
            chosen += [k for k in sorted(picks) if picks[k][1] == target][:1]
        by_call = [None if e is None else E.to_ints(e[i]) for e in elems_by_call]
        got = E.oracle_sums(ocfg, E.to_ints(st0[i]), tag0[i], idx0[i], script, by_call, chosen)
        for k in chosen:
            assert got[k] == picks[k][0], (i, k, picks[k][1])


def test_hash_rows_start_from_zero_with_edge_elements_only():
    """hash rows: a new sponge's first block is 0 or p - 1 only; later blocks come from the state after each permutation"""
    ocfg = O.make_config(O.BLS12_381_FR, 255, 2, 5, 8, 31)
    cr = cref.CRef(ocfg)
    p = ocfg.p
    msgs, digests, g = E.hash_rows(ocfg, 40, 7, 3, seed=5, c_port=cr)
    assert np.array_equal(digests, cr.hash_batch(msgs, 7, 3))
    for c, i, j, s, x, target in g.adds:
        if j < 2:
            assert s == 0 and x in (0, p - 1), (i, j)
    assert all(g.hits[k] > 0 for k in ("sum_p", "sum_pm1", "sum_pp1", "x_zero", "x_pm1")), g.hits
