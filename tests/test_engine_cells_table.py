"""The cell table of tests/engine_cells.py against the sources it claims to cover - no GPU.

The instantiations are COUNTED OUT OF sponge_amd/csrc/ (the widths of the window engines from PMX_MFMA_MIN_T / PMX_MFMA_MAX_T, the exponent
split of by_alpha and of window_engine_of and the two Montgomery steps by regular expression), so a new engine, exponent class or width fails
here until it has cells.  Every instantiation x row is either a cell or a named unreachable pair, the unreachable ones are exactly what the
launchers' own lines make so, and what the GPU test relies on - the p1 class of the two fields, a searched range for every grind cell, the
directed units, the window tables of every window cell's config - is asserted here, where the C port and the host build of the kernel
templates (tests/hostcheck) need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from sponge_amd import poseidon as P
from sponge_amd._lib import MODE_ABSORBING, MODE_SQUEEZING, PmxConfig
from oracle import cref
from oracle import poseidon_oracle as O

import engine_cells as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sponge_amd", "csrc")
HOSTCHECK = os.path.join(ROOT, "tests", "hostcheck")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def function_body(text, head):
    """the text from the regular expression `head` to the first line that is a lone closing brace"""
    m = re.search(head + r".*?\n\}", text, re.S)
    assert m, head
    return m.group(0)


def source_instantiations():
    """{(engine template, width or None, ALPHA, p1 or None)} as select_engine can return them, read out of the sources"""
    mfma, dev = source("pmx_mfma.hpp"), source("pmx_device.hip")
    lo = int(re.search(r"#define PMX_MFMA_MIN_T (\d+)", mfma).group(1))
    hi = int(re.search(r"#define PMX_MFMA_MAX_T (\d+)", mfma).group(1))
    by_alpha = function_body(dev, r"static const EngineOps \*by_alpha\(const DevConfig &c\) \{")
    alphas3 = [int(a) for a in re.findall(r"engine_ops<Engine<(\d+)>>", by_alpha)]
    select = function_body(dev, r"static const EngineOps \*select_engine\(")
    families = re.findall(r"by_alpha<(\w+)>\(c\)", select)
    assert "window_engine(c, t)" in select
    window_of = function_body(dev, r"static const EngineOps \*window_engine_of\(const DevConfig &c, uint32_t t\) \{")
    alphas2 = sorted({int(a) for a in re.findall(r"window_ops<(\d+), (?:false|true), P1>", window_of)})
    steps = sorted(set(re.findall(r"window_engine_of<(true|false)>\(c, t\)", function_body(dev, r"static const EngineOps \*window_engine\("))))
    assert len(alphas3) == len(set(alphas3)) and len(families) == len(set(families)) and alphas2 and steps
    out = {("HybridEngine", t, a, s == "true") for t in range(lo, hi + 1) for a in alphas2 for s in steps}
    out |= {(fam, None, a, None) for fam in families for a in alphas3}
    return out


def table_instantiations():
    name = {"window": "HybridEngine", "quad": "QuadEngine", "lds": "LdsEngine"}
    return [(name[i.family], i.t if i.family == "window" else None, E.template_alpha(i), i.p1 if i.family == "window" else None)
            for i in E.INSTANTIATIONS]


def test_the_table_has_the_instantiations_the_sources_can_select():
    src, tab = source_instantiations(), table_instantiations()
    assert len(tab) == len(set(tab)), "an instantiation is listed twice"
    assert set(tab) == src, (sorted(src - set(tab), key=str), sorted(set(tab) - src, key=str))
    assert len(E.INSTANTIATIONS) == len(src) == 34       # (what the sources hold today; the line above is the check)
    assert len({E.inst_id(i) for i in E.INSTANTIATIONS}) == len(E.INSTANTIATIONS)
    dev = source("pmx_device.hip")
    assert int(re.search(r"kQuadMaxUnits = (\d+);", dev).group(1)) == E.QUAD_MAX
    assert re.search(r"static bool quad_table\(const DevConfig &c, uint32_t t\) \{\s*return t == 3 &&", dev)
    assert all(i.t == 3 for i in E.INSTANTIATIONS if i.family == "quad")
    hi = int(re.search(r"#define PMX_MFMA_MAX_T (\d+)", source("pmx_mfma.hpp")).group(1))
    assert all(i.t > hi for i in E.INSTANTIATIONS if i.family == "lds"), "the run-time-width cells must lie beyond the window engines"


def test_the_rows_are_the_members_of_the_operation_table():
    ops = function_body(source("pmx_launch.hpp"), r"struct EngineOps \{")
    members = re.findall(r"hipError_t \(\*(\w+)\)\(", ops)
    assert tuple(members) == E.ROWS
    filled = re.search(r"static constexpr EngineOps ops = \{(.*?),\s*&Engine::lds_bytes", source("pmx_engine_launch.hpp"), re.S).group(1)
    assert tuple(re.findall(r"&L::(\w+)", filled)) == E.ROWS


def test_every_pair_is_a_cell_or_a_named_unreachable_pair_and_never_both():
    pairs = [(E.inst_id(i), r) for i in E.INSTANTIATIONS for r in E.ROWS]
    assert len(pairs) == len(set(pairs)) == 34 * 10
    assert set(E.UNREACHABLE) <= set(pairs)
    assert all(isinstance(reason, str) and len(reason) > 40 for reason in E.UNREACHABLE.values())
    for i in E.INSTANTIATIONS:
        for r in E.ROWS:
            c = E.cell(i, r)
            assert (c is None) == ((E.inst_id(i), r) in E.UNREACHABLE), (i, r)
            if c is not None:
                assert c.inst == i and c.row == r and c.rate + c.capacity == i.t
    assert len(E.cells()) + len(E.UNREACHABLE) == len(pairs)


def test_the_unreachable_pairs_are_what_the_launchers_make_unreachable():
    """Every row but compress_ary is launched for whatever engine the choice names.  launch_compress_ary refuses an arity beyond the rate and
    hands arity 2 to launch_compress, so an engine has a compress_ary cell iff one of its splits has rate >= 3: the quad engine's compress
    choice wants rate == 2 (quad_shape), every other engine takes any split of its width."""
    dev = source("pmx_device.hip")
    ary = function_body(dev, r"hipError_t launch_compress_ary\(")
    assert "if (arity < 2 || arity > c.rounds.rate) return hipErrorInvalidValue;" in ary
    assert "if (arity == 2) return launch_compress(c, t, in, out, n, st);" in ary
    assert re.search(r"quad_shape\(const DevConfig &c, uint32_t t\) \{ return quad_table\(c, t\) && c\.rounds\.capacity == 1 && c\.rounds\.rate == 2; \}", dev)
    select = function_body(dev, r"static const EngineOps \*select_engine\(")
    assert re.search(r"case PMX_OP_COMPRESS:.*?case PMX_OP_GRIND: quad = quad_shape\(c, t\); break;", select, re.S)
    level = function_body(dev, r"hipError_t launch_compress_level\(")
    assert "->compress_ary_bounded(" in level and "arity == 2" not in level      # the bounded twin runs at arity 2 too, the quad engine included
    for name in ("permute", "hash", "hash_strided", "compress", "grind", "absorb", "absorb_varlen", "squeeze"):
        body = function_body(dev, r"hipError_t launch_%s\(" % name)
        assert re.search(r"select_engine\(c, t, PMX_OP_\w+, n\)->%s\(" % name, body), name

    def max_rate(inst):
        return 2 if inst.family == "quad" else inst.t         # (rate t, capacity 0 is a split of every other engine)
    derived = {(E.inst_id(i), "compress_ary") for i in E.INSTANTIATIONS if max_rate(i) < 3}
    assert derived == set(E.UNREACHABLE)


def test_shapes_reach_the_engine_of_their_cell():
    for c in E.cells():
        i = c.inst
        if i.family == "quad":
            assert (c.rate, c.capacity) == (2, 1) and c.n == E.N_UNITS <= E.QUAD_MAX
        elif (c.rate, c.capacity) == (2, 1):
            assert i.family == "window" and i.t == 3 and c.n == E.QUAD_MAX + E.N_UNITS       # above the quad engine's range
        else:
            assert c.n == E.N_UNITS
        assert (c.rate, c.capacity) == (i.t - 1, 1) or (i.t == 3 and c.row == "compress_ary"), "one cell leaves the standard split"
        if c.row == "compress_ary":
            assert 3 <= c.arity <= c.rate and (c.arity == i.t - 1 or i.t == 3)
        if c.row == "compress_ary_bounded":
            leaves = E.inputs(c)["leaves"].shape[0]
            assert 2 <= c.arity <= c.rate and leaves == c.n * c.arity - 1 and -(-leaves // c.arity) == c.n and leaves % c.arity
        if c.row == "grind":
            assert E.GRIND_INDEX < c.rate
        op, n, length = E.engine_question(c)
        assert n == c.n and (length > 0) == (c.row in ("hash", "hash_strided") + E.DRIVER_ROWS)


def test_p1_is_derived_from_the_modulus_for_both_fields():
    assert E.p1_of(O.BLS12_381_FR) and O.BLS12_381_FR % 2**29 == 1
    assert not E.p1_of(O.BN254_FR) and O.BN254_FR % 2**28 == 1
    for i in E.INSTANTIATIONS:
        oc, pc = E.oracle_config(i, i.t - 1, 1), E.product_config(i, i.t - 1, 1)
        assert E.p1_of(oc.p) == i.p1 and pc.field.modulus == oc.p
        assert (oc.alpha, oc.full_rounds, oc.partial_rounds) == (pc.alpha, pc.full_rounds, pc.partial_rounds)
        assert oc.full_rounds == 8 and oc.partial_rounds in (31, 56, 57)
        if i.alpha_class == "generic":
            assert oc.alpha not in (5, 17) or (i.family == "window" and oc.alpha == 17)
        else:
            assert oc.alpha == int(i.alpha_class)
    generic = {(i.p1, E.alpha_of(i)) for i in E.INSTANTIATIONS if i.family == "window" and i.alpha_class == "generic"}
    assert generic == {(True, 17), (False, E.SMALL_ALPHA)}, "the reference's default on BLS, the small exponent on BN254"


@pytest.mark.parametrize("ident", [E.inst_id(i) for i in E.INSTANTIATIONS])
def test_every_grind_cell_searches(ident):
    """at least two accepted nonces in the range, the smallest beyond the first wave (workgroup): by the C port alone"""
    c = E.cell(E.BY_ID[ident], "grind")
    E.assert_grind_searches(c)
    bits, state, hits = E.grind_plan(c)
    assert state.shape == (c.inst.t, 4) and hits[0] >= (256 if c.n > E.QUAD_MAX else 64) and len(hits) >= 2
    # the rule once more through the C port's sponge: the first hit is accepted, its predecessor is not
    cr, oc = E.c_port(c.inst, c.rate, c.capacity), E.oracle_config(c.inst, c.rate, c.capacity)
    for nonce, accepted in ((hits[0], True), (hits[0] - 1, False)):
        s, m, ix = cr.sponge_absorb(state, MODE_ABSORBING, E.GRIND_INDEX, cref.elems_to_limbs([nonce], oc.p))
        _, _, _, out = cr.sponge_squeeze(s, m, ix, 1)
        assert (cref.limbs_to_elems(out, oc.p)[0] % (1 << bits) == 0) == accepted


def test_directed_units_are_in_range_distinct_and_in_the_batches():
    for i in E.INSTANTIATIONS:
        for row in ("permute", "hash", "compress", "compress_ary", "compress_ary_bounded", "squeeze"):
            c = E.cell(i, row)
            if c is None:
                continue
            oc = E.oracle_config(i, c.rate, c.capacity)
            vals = E.directed_values(c)
            assert all(0 <= v < oc.p for v in vals) and len(set(vals)) == 4, (E.inst_id(i), row)
            d = E.inputs(c)
            units = d["states"] if "states" in d else d["rows"] if "rows" in d else d["leaves"][:4 * c.arity].reshape(4, c.arity, 4)
            at = c.capacity if "states" in d else 0
            width = units.shape[1]
            got = [cref.limbs_to_elems(units[k], oc.p) for k in range(4)]
            assert got[0] == [0] * width and got[1] == [oc.p - 1] * width and got[2] == [1] * width
            assert (got[3][at] + oc.ark[0][c.capacity]) % oc.p == 0
            assert len({tuple(g) for g in got}) == 4


def test_driver_cells_hold_every_mode_and_every_row_length():
    for i in E.INSTANTIATIONS:
        c = E.cell(i, "absorb_varlen")
        tags, indices = E.modes(c)
        want = {(m, k) for m in (MODE_ABSORBING, MODE_SQUEEZING) for k in range(c.rate + 1)}
        assert set(zip(tags.tolist(), indices.tolist())) == want
        off = E.ragged_offsets(c)
        lengths = np.diff(off.astype(np.int64))
        assert set(lengths.tolist()) == set(range(2 * c.rate + 2)) and int(off[-1]) == E.inputs(c)["elems"].shape[0]
        # a row length meets more than one mode
        assert len({(int(l), int(m), int(k)) for l, m, k in zip(lengths, tags, indices)}) >= min(c.n, 4 * (c.rate + 1))


@pytest.fixture(scope="module")
def hc():
    subprocess.check_call(["make", "-C", HOSTCHECK, "all"], stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(HOSTCHECK, "libpmx_hostcheck.so"))
    for name in ("hc_permute_hybrid_mfma", "hc_permute_coop", "hc_permute_rt"):
        getattr(lib, name).argtypes = [ctypes.POINTER(PmxConfig), ctypes.c_void_p, ctypes.c_size_t]
    return lib


@pytest.mark.parametrize("ident", [E.inst_id(i) for i in E.INSTANTIATIONS])
def test_the_config_of_every_instantiation_has_its_engines_tables_on_the_host_build(hc, ident):
    """prepare() on the host: the window tables exist for every window cell's config (a zero in the window algebra would drop it to the
    run-time-width engine - the GPU test asserts the engine again before it calls), the quad engine's for every quad cell's; and the host
    build of that schedule permutes the cell's first units - the directed ones - like the C port."""
    inst = E.BY_ID[ident]
    c = E.cell(inst, "permute")
    cfg = E.product_config(inst, c.rate, c.capacity)
    fn = {"window": hc.hc_permute_hybrid_mfma, "quad": hc.hc_permute_coop, "lds": hc.hc_permute_rt}[inst.family]
    states = np.array(E.inputs(c)["states"][:8])
    want = E.c_port(inst, c.rate, c.capacity).permute_batch(states, threads=1)
    pc = P.c_config(cfg)
    assert fn(ctypes.byref(pc), states.ctypes.data, states.shape[0]) == 0, "the config has no tables for the intended engine"
    assert np.array_equal(states, want)
