"""The table  engine instantiation x operation -> cell  behind tests/test_engine_cells_table.py (CPU) and tests/test_gpu_engine_cells.py.

select_engine (sponge_amd/csrc/pmx_device.hip) can return 34 operation tables (pmx_launch.hpp: EngineOps), each with ten launchable rows,
every pair a kernel of its own.  This module declares one CELL per pair - the config, the shape and the seeded inputs of one call through a
public entry point, and the expected value of every output from the oracle's C restatement (oracle/cref) - or names the pair UNREACHABLE
with the line of the launchers that makes it so.  Nothing here opens a GPU, and nothing here asks the library under test for an expected
value: the product is used for its fields' descriptions, for the constants of the PRODUCT's own LFSR (as gpu_helpers.product_config) and,
in run(), for the call itself; the C port is fed the ORACLE's constants.

Instantiations are (family, t, alpha_class, p1):
  window   HybridEngine / HybridEngineP1   t = 3 .. 9 x alpha_class in {5, generic} x p1 in {True, False}.  The engine string does not show
           the Montgomery step, so p1 is DERIVED from the modulus (p % 2^29 == 1: BLS12-381 Fr is, BN254 Fr is not; p1_of).  On these
           engines alpha = 17 belongs to generic: the BLS cells use it (the reference's default), the BN254 ones the small exponent.
  quad     QuadEngine<5 | 17 | 0>          t = 3, split (rate 2, capacity 1), at most 32768 units
  lds      LdsEngine<5 | 17 | 0>           t = 10 (rate 9, capacity 1): beyond the window engines' widths

Batches are n = 257 units (one whole workgroup and one lane); the window engines of t = 3 with the (2, 1) split are reached only above the
quad engine's range, there n = 32768 + 257.  The first four units of every batch are directed (all 0, all p - 1, all 1, one whose element at
lane `capacity` cancels the first round constant so that the first S-box sees 0), the rest seeded synth.random_elements."""
import collections
import ctypes
import functools

import numpy as np

import sponge_amd as S
from sponge_amd import _lib, synth
from sponge_amd._lib import MATRIX_COL_MAJOR, MATRIX_ROW_MAJOR, MODE_ABSORBING, MODE_SQUEEZING
from oracle import cref
from oracle import poseidon_oracle as O

import merkle_ary_oracle as MA
import merkle_ragged_oracle as MR

ROWS = ("permute", "hash", "hash_strided", "compress", "compress_ary", "compress_ary_bounded", "grind", "absorb", "absorb_varlen", "squeeze")
DRIVER_ROWS = ("absorb", "absorb_varlen", "squeeze")

QUAD_MAX = 32768          # pmx_device.hip: kQuadMaxUnits
N_UNITS = 257             # one workgroup of 256 lanes and one lane
WINDOW_T = range(3, 10)   # checked against PMX_MFMA_MIN_T / PMX_MFMA_MAX_T by tests/test_engine_cells_table.py
LDS_T = 10
FULL_ROUNDS = 8
SMALL_ALPHA = 3           # the generic exponent that is neither 5 nor 17 (3, then 7: the first for which the intended engine answers)

# (product field, modulus, its bit size) by p1
FIELD_OF_P1 = {True: (S.BLS12_381_FR, O.BLS12_381_FR, 255), False: (S.BN254_FR, O.BN254_FR, 254)}

Inst = collections.namedtuple("Inst", "family t alpha_class p1")
# one call: the split, the units the engine choice sees, the children per parent (tree rows; 0 elsewhere)
Cell = collections.namedtuple("Cell", "inst row rate capacity n arity")


def p1_of(p):
    """the Montgomery step the window engines take for modulus p (pmx_device.hip: window_engine, field_unit_low_limb)"""
    return p % 2**29 == 1


assert p1_of(O.BLS12_381_FR) and not p1_of(O.BN254_FR)
assert all(p1_of(FIELD_OF_P1[k][1]) == k and FIELD_OF_P1[k][0].modulus == FIELD_OF_P1[k][1] for k in (True, False))


def inst_id(inst):
    alpha = inst.alpha_class if inst.alpha_class == "generic" else "a" + inst.alpha_class
    if inst.family == "window":
        return "window-t%d-%s-%s" % (inst.t, alpha, "p1" if inst.p1 else "p0")
    return "%s-%s" % (inst.family, alpha)


INSTANTIATIONS = tuple(
    [Inst("window", t, a, p1) for t in WINDOW_T for a in ("5", "generic") for p1 in (True, False)]
    + [Inst("quad", 3, a, True) for a in ("5", "17", "generic")]
    + [Inst("lds", LDS_T, a, True) for a in ("5", "17", "generic")])
BY_ID = {inst_id(i): i for i in INSTANTIATIONS}

# pairs no public call reaches, each with the line that makes it so.  tests/test_engine_cells_table.py derives the same set from the sources.
UNREACHABLE = {
    (inst_id(i), "compress_ary"): "quad_shape wants rate == 2 and launch_compress_ary hands arity 2 to launch_compress (pmx_device.hip: "
                                  "`if (arity == 2) return launch_compress(c, t, in, out, n, st);`): no arity is left for the quad engine"
    for i in INSTANTIATIONS if i.family == "quad"}


def alpha_of(inst):
    if inst.alpha_class != "generic":
        return int(inst.alpha_class)
    if inst.family == "window" and inst.p1:
        return 17
    return SMALL_ALPHA


def partial_rounds_of(inst):
    """the partial-round counts the project's configs use at that width (tests/golden/config_pins.json, tests/merkle_ary_oracle.py)"""
    if inst.t == 3:
        return 31 if inst.p1 else 57
    return 56 if inst.t in (4, 5) else 57


def template_alpha(inst):
    """the ALPHA template argument of the engine's name"""
    if inst.family == "window":
        return 5 if inst.alpha_class == "5" else 0
    return 0 if inst.alpha_class == "generic" else int(inst.alpha_class)


def intended_engine(inst, row):
    """what pmx_ctx_engine_info must answer before the call of that row: (prefix, the driver rows run as passes)"""
    a = template_alpha(inst)
    if inst.family == "window":
        return b"HybridEngine<%d,%d," % (inst.t, a), row in DRIVER_ROWS
    return (b"QuadEngine<%d>" if inst.family == "quad" else b"LdsEngine<%d>") % a, False


def engine_matches(inst, row, name):
    prefix, passes = intended_engine(inst, row)
    if inst.family != "window":
        return name == prefix
    return name.startswith(prefix) and name.endswith(b" x passes") == passes


def cell(inst, row):
    """the Cell of a pair, or None for an UNREACHABLE one"""
    if (inst_id(inst), row) in UNREACHABLE:
        return None
    rate, capacity, n, arity = inst.t - 1, 1, N_UNITS, 0
    if inst.family == "window" and inst.t == 3:
        n = QUAD_MAX + N_UNITS                      # the (2, 1) split below that is the quad engine's
    if row == "compress":
        arity = 2
    elif row == "compress_ary":
        arity = rate
        if inst.t == 3:                             # arity >= 3 at t = 3 exists for the split (rate 3, capacity 0) only, the one cell
            rate, capacity, arity, n = 3, 0, 3, N_UNITS   # that leaves the standard split; that split never meets the quad engine
    elif row == "compress_ary_bounded":
        arity = rate                                # (2 at t = 3): n parents at the bottom level, the last of them one child short
    return Cell(inst, row, rate, capacity, n, arity)


def cells():
    return [c for c in (cell(i, r) for i in INSTANTIATIONS for r in ROWS) if c is not None]


def seed_of(c, salt=0):
    return 0xCE110000 + 4096 * INSTANTIATIONS.index(c.inst) + 64 * ROWS.index(c.row) + salt


# ---- configs --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_config(inst, rate, capacity):
    _, p, bits = FIELD_OF_P1[inst.p1]
    base = O.make_config(p, bits, inst.t - 1, alpha_of(inst), FULL_ROUNDS, partial_rounds_of(inst))
    if (rate, capacity) == (base.rate, base.capacity):
        return base
    return O.PoseidonConfig(p, base.full_rounds, base.partial_rounds, base.alpha, base.ark, base.mds, rate, capacity)


@functools.lru_cache(maxsize=None)
def c_port(inst, rate, capacity):
    return cref.CRef(oracle_config(inst, rate, capacity))


@functools.lru_cache(maxsize=None)
def product_config(inst, rate, capacity):
    """constants from the PRODUCT's own LFSR (host code of the library; no GPU)"""
    f = FIELD_OF_P1[inst.p1][0]
    base = S.poseidon_config_from_lfsr(f, inst.t - 1, alpha_of(inst), FULL_ROUNDS, partial_rounds_of(inst))
    if (rate, capacity) == (base.rate, base.capacity):
        return base
    return S.PoseidonConfig(f, base.full_rounds, base.partial_rounds, base.alpha, base.mds, base.ark, rate, capacity)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def directed(c, units, width, cancel_at):
    """units [n][width][4] seeded, the first four directed: every element 0, p - 1, 1, and one unit whose element `cancel_at` is minus the
    first round constant of lane `capacity` (the lane that element enters), so that the lane's first S-box input is 0"""
    oc = oracle_config(c.inst, c.rate, c.capacity)
    p = oc.p
    units[0] = 0
    units[1] = cref.elems_to_limbs([p - 1], p)[0]
    units[2] = cref.elems_to_limbs([1], p)[0]
    units[3, cancel_at] = cref.elems_to_limbs([(p - oc.ark[0][c.capacity]) % p], p)[0]
    return units


def directed_values(c):
    """the four directed elements as canonical integers (for the table test: in range and distinct)"""
    oc = oracle_config(c.inst, c.rate, c.capacity)
    return [0, oc.p - 1, 1, (oc.p - oc.ark[0][c.capacity]) % oc.p]


def modes(c):
    """(tags, indices) [n]: every mode Absorbing{0 .. rate}, Squeezing{0 .. rate} present, shifted by one every 2 rate + 2 units so that
    the ragged rows' lengths (the same period) meet every mode"""
    i = np.arange(c.n)
    period = 2 * c.rate + 2
    k = (i + i // period) % period
    tags = np.where(k <= c.rate, MODE_ABSORBING, MODE_SQUEEZING).astype(np.uint32)
    return tags, (k % (c.rate + 1)).astype(np.uint32)


def ragged_offsets(c):
    """offsets [n + 1] of rows whose lengths cycle 0 .. 2 rate + 1 (empty rows included)"""
    lengths = np.arange(c.n) % (2 * c.rate + 2)
    off = np.zeros(c.n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lengths)
    return off


@functools.lru_cache(maxsize=None)
def inputs(c):
    """the call's arrays by name; read-only (run() copies what the library writes)"""
    f = FIELD_OF_P1[c.inst.p1][0]
    t, rate, cap, n = c.rate + c.capacity, c.rate, c.capacity, c.n

    def rand(count, salt=0):
        return synth.random_elements(f, count, seed=seed_of(c, salt))

    d = {}
    if c.row == "permute":
        d["states"] = directed(c, rand(n * t).reshape(n, t, 4), t, cap)
    elif c.row in ("hash", "hash_strided"):
        d["rows"] = directed(c, rand(n * (rate + 1)).reshape(n, rate + 1, 4), rate + 1, 0)
    elif c.row in ("compress", "compress_ary"):
        d["leaves"] = directed(c, rand(n * c.arity).reshape(n, c.arity, 4), c.arity, 0).reshape(n * c.arity, 4)
    elif c.row == "compress_ary_bounded":
        full = directed(c, rand(n * c.arity).reshape(n, c.arity, 4), c.arity, 0).reshape(n * c.arity, 4)
        d["leaves"] = np.ascontiguousarray(full[:n * c.arity - 1])             # the last parent is one child short
    elif c.row == "grind":
        pass                                                                   # grind_plan chooses the state
    else:
        d["states"] = directed(c, rand(n * t).reshape(n, t, 4), t, cap)
        d["tags"], d["indices"] = modes(c)
        if c.row == "absorb":
            d["elems"] = directed(c, rand(n * (2 * rate + 1), 1).reshape(n, 2 * rate + 1, 4), 2 * rate + 1, 0)
            d["elems"][3] = 0       # the fourth sponge absorbs zeros: whatever its mode, its first permutation meets the cancelling lane
        elif c.row == "absorb_varlen":
            d["offsets"] = ragged_offsets(c)
            d["elems"] = rand(int(d["offsets"][-1]), 1)
            d["elems"][int(d["offsets"][3]):int(d["offsets"][4])] = 0
    for a in d.values():
        a.setflags(write=False)
    return d


# ---- grind: bits and the state seed per cell, from the oracle alone ----------------------------------------------------------------
GRIND_INDEX = 1      # Absorbing{1}: the nonce enters at state[capacity + 1] (every cell has rate >= 2)


def grind_state(c, seed):
    f = FIELD_OF_P1[c.inst.p1][0]
    return synth.random_elements(f, c.rate + c.capacity, seed=seed_of(c, 16 + seed)).reshape(c.rate + c.capacity, 4)


def grind_digests(oc, cr, base, tag, index, first, count):
    """the acceptance rule of tests/grind_oracle.py for any config: the canonical integer of the first squeezed element for every nonce of
    [first, first + count).  An Absorbing{rate} or Squeezing sponge permutes first (mod.rs:239-252), F::from(v) is added into
    state[capacity + index], the squeeze permutes and hands out state[capacity]."""
    p = oc.p
    base = np.array(base, dtype=np.uint64)
    if tag == MODE_SQUEEZING or index == oc.rate:
        base = cr.permute_batch(base[None], threads=1)[0]
        index = 0
    at = oc.capacity + index
    states = np.repeat(base[None], count, axis=0)
    lane = O.from_limbs([int(x) for x in base[at]])
    r = (1 << 256) % p
    for k in range(count):
        states[k, at] = np.array(O.to_limbs((lane + (first + k) * r) % p), dtype=np.uint64)   # += F::from(v): residues add (mod.rs:128)
    out = cr.permute_batch(states, threads=0)
    return cref.limbs_to_elems(out[:, oc.capacity], p)


def grind_min_first_hit(c):
    """the smallest accepted nonce must lie beyond the first wave - beyond the first workgroup where the launch has 130 of them"""
    return 256 if c.n > QUAD_MAX else 64


@functools.lru_cache(maxsize=None)
def grind_plan(c):
    """(bits, state [t][4], the oracle's accepted nonces of [0, n), ascending): the first state seed of 0 .. 31 for which the range holds at
    least two accepted nonces and the smallest is not in the first wave (workgroup); bits so that about four are expected"""
    assert c.row == "grind"
    bits = (c.n // 4).bit_length() - 1                  # 257 -> 6 (one nonce in 64), 33025 -> 13 (one in 8192)
    oc, cr = oracle_config(c.inst, c.rate, c.capacity), c_port(c.inst, c.rate, c.capacity)
    for seed in range(32):
        state = grind_state(c, seed)
        d = grind_digests(oc, cr, state, MODE_ABSORBING, GRIND_INDEX, 0, c.n)
        hits = [k for k in range(c.n) if d[k] & ((1 << bits) - 1) == 0]
        if len(hits) >= 2 and hits[0] >= grind_min_first_hit(c):
            state.setflags(write=False)
            return bits, state, tuple(hits)
    raise AssertionError("no state seed gives %s a searched range: it would pass because nothing was searched" % (c,))


def assert_grind_searches(c):
    """both conditions, asserted before the call"""
    bits, _, hits = grind_plan(c)
    assert len(hits) >= 2, (c, hits)
    assert hits[0] >= grind_min_first_hit(c) and hits[-1] < c.n, (c, hits)
    assert 0 < bits < 30


# ---- expected values: the C port, every unit in full ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected(c):
    """the outputs by name (what run() returns under the same names)"""
    cr = c_port(c.inst, c.rate, c.capacity)
    d = inputs(c)
    rate, n = c.rate, c.n
    if c.row == "permute":
        return {"states": cr.permute_batch(d["states"], threads=0)}
    if c.row == "hash":
        return {"out": cr.hash_batch(d["rows"], rate + 1, 2, threads=0)}
    if c.row == "hash_strided":
        leaves = cr.hash_batch(d["rows"], rate + 1, 1, threads=0).reshape(n, 4)
        return {"leaves_row_major": leaves, "leaves_col_major": leaves}
    if c.row == "compress":          # n trees of two leaves by the C port's own tree builder; level-major: every leaf, then every root
        roots = np.stack([cr.merkle(d["leaves"][2 * i:2 * i + 2])[2] for i in range(n)])
        return {"nodes": np.concatenate([d["leaves"], roots]), "roots": roots}
    if c.row == "compress_ary":
        nodes = MA.forest(cr, d["leaves"], n, c.arity)
        return {"nodes": nodes, "roots": nodes[-n:]}
    if c.row == "compress_ary_bounded":
        nodes = MR.tree(cr, d["leaves"], c.arity)
        return {"nodes": nodes, "root": nodes[-1]}
    if c.row == "grind":
        _, _, hits = grind_plan(c)
        return {"found": 1, "nonce": hits[0]}
    if c.row == "absorb":
        off = np.arange(n + 1, dtype=np.uint64) * np.uint64(2 * rate + 1)
        s, tg, ix = cr.sponge_absorb_each(d["states"], d["tags"], d["indices"], d["elems"], off)
        return {"states": s, "tags": tg, "indices": ix}
    if c.row == "absorb_varlen":
        s, tg, ix = cr.sponge_absorb_each(d["states"], d["tags"], d["indices"], d["elems"], d["offsets"])
        return {"states": s, "tags": tg, "indices": ix}
    s, tg, ix, out = cr.sponge_squeeze_each(d["states"], d["tags"], d["indices"], 2 * rate + 1)
    return {"states": s, "tags": tg, "indices": ix, "out": out}


# ---- the call (GPU) ---------------------------------------------------------------------------------------------------------------
def engine_question(c):
    """(op, n, len) of pmx_ctx_engine_info for the launch of the cell's row (the bottom level of a tree)"""
    op = {"permute": _lib.OP_PERMUTE, "hash": _lib.OP_HASH, "hash_strided": _lib.OP_HASH, "compress": _lib.OP_COMPRESS,
          "compress_ary": _lib.OP_COMPRESS, "compress_ary_bounded": _lib.OP_COMPRESS, "grind": _lib.OP_GRIND, "absorb": _lib.OP_ABSORB,
          "absorb_varlen": _lib.OP_ABSORB, "squeeze": _lib.OP_SQUEEZE}[c.row]
    length = {"hash": c.rate + 1, "hash_strided": c.rate + 1, "absorb": 2 * c.rate + 1, "absorb_varlen": 2 * c.rate + 1,
              "squeeze": 2 * c.rate + 1}.get(c.row, 0)
    return op, c.n, length


def engine_answer(c):
    """the engine string the library names for the cell's launch"""
    op, n, length = engine_question(c)
    info = _lib.PmxEngineInfo()
    ctx = product_config(c.inst, c.rate, c.capacity).context(0)
    _lib.check(_lib.lib().pmx_ctx_engine_info(ctx._h, op, n, length, ctypes.byref(info)))
    return info.engine


def run(c):
    """the cell's call through its public entry point: the outputs under the names of expected()"""
    ctx = product_config(c.inst, c.rate, c.capacity).context(0)
    d = inputs(c)
    rate, n = c.rate, c.n
    if c.row == "permute":
        return {"states": ctx.permute_batch(d["states"])}
    if c.row == "hash":
        return {"out": ctx.hash_batch(d["rows"], rate + 1, 2)}
    if c.row == "hash_strided":
        by_column = np.ascontiguousarray(d["rows"].transpose(1, 0, 2))
        return {"leaves_row_major": ctx.matrix_leaves(np.ascontiguousarray(d["rows"]), n, rate + 1, MATRIX_ROW_MAJOR),
                "leaves_col_major": ctx.matrix_leaves(by_column, n, rate + 1, MATRIX_COL_MAJOR)}
    if c.row == "compress":
        nodes, roots = ctx.merkle_2to1_forest(d["leaves"], n)
        return {"nodes": nodes, "roots": roots}
    if c.row == "compress_ary":
        nodes, roots = ctx.merkle_ary_forest(d["leaves"], n, c.arity)
        return {"nodes": nodes, "roots": roots}
    if c.row == "compress_ary_bounded":
        nodes, root = ctx.merkle_ragged(d["leaves"], c.arity)
        return {"nodes": nodes, "root": root}
    if c.row == "grind":
        bits, state, _ = grind_plan(c)
        nonce, found = ctypes.c_uint64(0), ctypes.c_int(0)
        st = np.array(state)
        _lib.check(_lib.lib().pmx_sponge_grind(ctx._h, ctypes.c_void_p(st.ctypes.data), MODE_ABSORBING, GRIND_INDEX, bits, 0, n,
                                               ctypes.byref(nonce), ctypes.byref(found)))
        assert st.tobytes() == state.tobytes(), "the caller's state was modified"
        return {"found": found.value, "nonce": nonce.value}
    states, tags, indices = np.array(d["states"]), np.array(d["tags"]), np.array(d["indices"])
    out = {"states": states, "tags": tags, "indices": indices}
    if c.row == "absorb":
        ctx.sponge_absorb_batch(states, tags, indices, np.ascontiguousarray(d["elems"]), 2 * rate + 1)
    elif c.row == "absorb_varlen":
        ctx.sponge_absorb_varlen_batch(states, tags, indices, d["elems"], d["offsets"])
    else:
        out["out"] = ctx.sponge_squeeze_batch(states, tags, indices, 2 * rate + 1)
    return out


def differences(got, want):
    """names of the outputs that differ from the C port in any limb or word"""
    assert set(got) == set(want)
    return [k for k in sorted(want) if not np.array_equal(np.asarray(got[k]), np.asarray(want[k]))]
