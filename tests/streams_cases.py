"""The case tables of tests/test_gpu_streams.py: one small call of every single-device *_dev entry point of include/poseidon_mi355x.h per
engine cell, its buffers, and what the oracle's C port (oracle/cref) makes of them.

A case names an entry point, a config label of tests/test_gpu_footprint.py and a shape.  data(case, variant) gives its buffers - name ->
(initial content, role), roles as in tests/arena.py - and the expected content of every out / inout buffer, computed from the C port once
per (case, variant) and cached read-only.  Variant 1 is the same shape with other values and other index contents (the second input set
of the capture tests).  invoke() makes the call on the current torch stream, through the dispatcher of tests/test_gpu_footprint.py where
it has the entry.  Nothing here synchronises or compares."""
import ctypes
import functools
from collections import namedtuple

import numpy as np

import sponge_amd as S
from sponge_amd import _lib, synth

import merkle_ary_oracle as MA
import merkle_ragged_oracle as MR
import test_gpu_footprint as FP
import test_gpu_squeeze_bytes as SB

Case = namedtuple("Case", "entry label shape")

CELLS = [("t3", 257), ("t3", 32769), ("t9-bn254", 257)]        # quad engine, window engine of t = 3, window engine of t = 9
CELLS_PERMUTE = CELLS + [("lds-t16", 257)]                      # and the run-time-width engine
K_PATHS = 65
BIG_TREE = 1 << 17                                               # level 1 is 65536 compressions: the window engine, then the quad kernels

# the entries whose header text allows capture into a graph, and those it excludes (with the header's reason)
CAPTURABLE = ["pmx_permute_batch_dev", "pmx_hash_batch_dev", "pmx_merkle_2to1_dev", "pmx_merkle_2to1_forest_dev", "pmx_merkle_verify_paths_dev",
              "pmx_merkle_ary_dev", "pmx_merkle_ary_forest_dev", "pmx_merkle_ary_paths_dev", "pmx_merkle_ary_verify_paths_dev",
              "pmx_merkle_ary_update_dev", "pmx_merkle_ragged_dev", "pmx_merkle_ragged_paths_dev", "pmx_merkle_ragged_verify_paths_dev",
              "pmx_merkle_ragged_update_dev"]
NOT_CAPTURABLE = {
    "pmx_sponge_absorb_batch_dev": "pass lists in the context's per-stream pool: may call hipMalloc",
    "pmx_sponge_squeeze_batch_dev": "pass lists in the context's per-stream pool: may call hipMalloc",
    "pmx_sponge_absorb_varlen_batch_dev": "pass lists in the context's per-stream pool: may call hipMalloc",
    "pmx_hash_varlen_batch_dev": "fresh states, mode words and pass lists in the context's per-stream pool: may call hipMalloc",
    "pmx_sponge_squeeze_bytes_batch_dev": "native elements pass through a scratch block of the per-stream pool: may call hipMalloc",
    "pmx_sponge_squeeze_bits_batch_dev": "native elements pass through a scratch block of the per-stream pool: may call hipMalloc",
}
OUT_OF_SCOPE = {name: "enqueues on the device group's own streams (pmx_mgpu_stream), not on a stream of the caller"
                for name in ("pmx_mgpu_permute_shards_dev", "pmx_mgpu_all_gather_dev", "pmx_mgpu_gather_dev", "pmx_mgpu_permute_gather_dev",
                             "pmx_mgpu_merkle_2to1_dev")}


def _rate(label):
    return FP.CONFIGS[label][1]


def _cases():
    out = []
    for label, n in CELLS_PERMUTE:
        r = _rate(label)
        out.append(Case("pmx_permute_batch_dev", label, (("n", n),)))
        out.append(Case("pmx_hash_batch_dev", label, (("n", n), ("in_len", r + 2), ("out_len", r + 1))))
    for label, n in CELLS:
        r = _rate(label)
        ub, ubits = SB._units(FP.FIELD[FP.CONFIGS[label][0]][0].modulus)
        # 2 rate + 1 elements: at least three launches of the pass form, both lists in use
        out.append(Case("pmx_sponge_absorb_batch_dev", label, (("n", n), ("in_len", 2 * r + 1))))
        out.append(Case("pmx_sponge_squeeze_batch_dev", label, (("n", n), ("out_len", 2 * r + 1))))
        out.append(Case("pmx_sponge_absorb_varlen_batch_dev", label, (("n", n),)))
        out.append(Case("pmx_hash_varlen_batch_dev", label, (("n", n), ("out_len", r + 1))))
        out.append(Case("pmx_sponge_squeeze_bytes_batch_dev", label, (("n", n), ("length", 2 * r * ub + 5))))     # E = 2 rate + 1 elements
        out.append(Case("pmx_sponge_squeeze_bits_batch_dev", label, (("n", n), ("length", 2 * r * ubits + 5))))
    for label, m in (("t3", 512), ("t3", BIG_TREE), ("t9-bn254", 512)):
        out.append(Case("pmx_merkle_2to1_dev", label, (("n_leaves", m),)))
    for label, n_trees, m in (("t3", 5, 64), ("t3", 9, 8192), ("t9-bn254", 5, 64)):      # 9 x 8192: level 1 is 36864 compressions
        out.append(Case("pmx_merkle_2to1_forest_dev", label, (("n_trees", n_trees), ("leaves_per_tree", m))))
    for label in ("t3", "t9-bn254"):
        out.append(Case("pmx_merkle_verify_paths_dev", label, (("n_leaves", 512), ("k", K_PATHS))))
    a, m = 8, 512
    out.append(Case("pmx_merkle_ary_dev", "t9-bn254", (("arity", a), ("n_leaves", m))))
    out.append(Case("pmx_merkle_ary_forest_dev", "t9-bn254", (("arity", a), ("n_trees", 3), ("leaves_per_tree", 64))))
    out.append(Case("pmx_merkle_ary_paths_dev", "t9-bn254", (("arity", a), ("n_leaves", m), ("k", K_PATHS))))
    out.append(Case("pmx_merkle_ary_verify_paths_dev", "t9-bn254", (("arity", a), ("n_leaves", m), ("k", K_PATHS))))
    for k in (5, m // a):           # gather / compress / scatter levels; k = the parents of level 1: whole levels from the first one on
        out.append(Case("pmx_merkle_ary_update_dev", "t9-bn254", (("arity", a), ("n_leaves", m), ("k", k))))
    for label, a, m in (("t9-bn254", 8, 1000), ("t3", 2, 1000)):
        out.append(Case("pmx_merkle_ragged_dev", label, (("arity", a), ("n_leaves", m))))
        out.append(Case("pmx_merkle_ragged_paths_dev", label, (("arity", a), ("n_leaves", m), ("k", K_PATHS))))
        out.append(Case("pmx_merkle_ragged_verify_paths_dev", label, (("arity", a), ("n_leaves", m), ("k", K_PATHS))))
        for k in (5, -(-m // a)):
            out.append(Case("pmx_merkle_ragged_update_dev", label, (("arity", a), ("n_leaves", m), ("k", k))))
    return out


CASES = _cases()


def case_id(case):
    return "-".join([case.entry[4:-4], case.label] + [f"{k}{v}" for k, v in case.shape])


def is_big(case):
    return dict(case.shape).get("n_leaves") == BIG_TREE


# ---- the engines of a case: (op, units, len) of every launch that runs on a permutation engine -----------------------------------------
def _update_units(widths, k):
    """pmx_merkle_ary_update_dev / pmx_merkle_ragged_update_dev: k rows per level while k is below the level's parents, whole levels after"""
    units = []
    for level in range(len(widths) - 1):
        if k >= widths[level + 1]:
            return units + widths[level + 1:]
        units.append(k)
    return units


def launches(case):
    s, r = dict(case.shape), _rate(case.label)
    e = case.entry
    a = s.get("arity", 2)
    if e == "pmx_permute_batch_dev":
        return [(_lib.OP_PERMUTE, s["n"], 0)]
    if e == "pmx_hash_batch_dev":
        return [(FP._hash_op(case.label, s["in_len"], s["out_len"]), s["n"], s["in_len"])]
    if e == "pmx_sponge_absorb_batch_dev":
        return [(_lib.OP_ABSORB, s["n"], s["in_len"])]
    if e == "pmx_sponge_squeeze_batch_dev":
        return [(_lib.OP_SQUEEZE, s["n"], s["out_len"])]
    if e == "pmx_sponge_absorb_varlen_batch_dev":
        return [(_lib.OP_ABSORB, s["n"], 5 * r)]
    if e == "pmx_hash_varlen_batch_dev":
        return [(_lib.OP_ABSORB, s["n"], 5 * r), (_lib.OP_SQUEEZE, s["n"], s["out_len"])]
    if e in ("pmx_sponge_squeeze_bytes_batch_dev", "pmx_sponge_squeeze_bits_batch_dev"):
        return [(_lib.OP_SQUEEZE, s["n"], 2 * r + 1)]
    if e in ("pmx_merkle_2to1_dev", "pmx_merkle_ary_dev", "pmx_merkle_ragged_dev"):
        return [(_lib.OP_COMPRESS, w, a) for w in MR.widths(s["n_leaves"], a)[1:]]
    if e in ("pmx_merkle_2to1_forest_dev", "pmx_merkle_ary_forest_dev"):
        return [(_lib.OP_COMPRESS, w * s["n_trees"], a) for w in MR.widths(s["leaves_per_tree"], a)[1:]]
    if e.endswith("verify_paths_dev"):
        return [(_lib.OP_COMPRESS, s["k"], a)]
    if e.endswith("update_dev"):
        return [(_lib.OP_COMPRESS, u, a) for u in _update_units(MR.widths(s["n_leaves"], a), s["k"])]
    assert e.endswith("paths_dev")      # a gather: no permutation engine
    return []


def engine_info(label, op, units, length):
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(FP._config(label)[1].context()._h, op, units, length, ctypes.byref(info)))
    return info


def assert_engines(case):
    """the engine of every launch of the case, asked of pmx_ctx_engine_info and asserted against the table of tests/test_gpu_footprint.py;
    returns the cells (tests/test_gpu_footprint.py: _cell) the case runs on"""
    cells = set()
    for op, units, length in launches(case):
        info = engine_info(case.label, op, units, length)
        want = FP._expected_engine(case.label, units)
        assert info.engine.startswith(want), (case_id(case), units, info.engine, want)
        if want.startswith(b"HybridEngine") and op in (_lib.OP_ABSORB, _lib.OP_SQUEEZE):
            assert b"passes" in info.engine, (case_id(case), info.engine)
            if length >= 2 * _rate(case.label) + 1:      # three launches or more: both lists of the pass form are in use
                assert info.launches >= 3, (case_id(case), info.engine, info.launches)
        cells.add(FP._cell(case.label, units))
    return cells


# ---- inputs and the C port's answers ------------------------------------------------------------------------------------------------------
def poison(shape, dtype, seed):
    rng = np.random.default_rng(0xBAD0000 + seed)
    count = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    return rng.integers(0, 256, count, dtype=np.uint8).view(dtype).reshape(shape)


def _sponges(f, t, r, n, seed):
    """half of the sponges Absorbing in the middle of the rate, half Squeezing at any index"""
    rng = np.random.default_rng(seed)
    st = synth.random_elements(f, n * t, seed=seed + 1).reshape(n, t, 4)
    tag = (np.arange(n) % 2).astype(np.uint32)
    idx = np.where(tag == S.MODE_ABSORBING, max(r // 2, 1), rng.integers(0, r + 1, n)).astype(np.uint32)
    return st, tag, idx


def _sponge_bufs(st, tag, idx):
    return {"d_states": (st, "inout"), "d_mode_tag": (tag, "inout"), "d_mode_index": (idx, "inout")}


def _absorbed(cr, st, tag, idx, elems, offsets):
    got = cr.sponge_absorb_each(st, tag, idx, elems, offsets)
    return {"d_states": got[0], "d_mode_tag": got[1], "d_mode_index": got[2]}


def _squeezed(cr, st, tag, idx, count):
    """(elements [n][count][4], the sponges afterwards as expected buffers)"""
    got = cr.sponge_squeeze_each(st, tag, idx, count)
    return got[3], {"d_states": got[0], "d_mode_tag": got[1], "d_mode_index": got[2]}


def _distinct(m, k, seed):
    """k distinct leaf indices, the last leaf and leaf 0 first"""
    picks = list(dict.fromkeys([m - 1, 0] + [int(x) for x in np.random.default_rng(seed).permutation(m)]))[:k]
    return np.array(picks, dtype=np.uint64)


def _tree_family(case):
    """(oracle module, arity, tree builder, cached tree) of a tree case"""
    s = dict(case.shape)
    ragged = "ragged" in case.entry
    M = MR if ragged else MA
    return M, s.get("arity", 2), s


def _opening(case, seed, variant):
    """k openings of the case's tree, one of them corrupted: (leaves, indices, good paths, paths with the corruption, root, verdicts)"""
    M, a, s = _tree_family(case)
    f, cfg, cr = FP._config(case.label)
    m, k = s["n_leaves"], s["k"]
    leaves, nodes = M.cached_tree(case.label, a, m)
    idx = M.path_indices(m, a, k, seed=seed)
    assert 0 in idx and m - 1 in idx
    paths = M.open_paths(nodes, m, a, idx)
    bad = paths.copy()
    full = np.nonzero(idx < np.uint64(m - 2 * a))[0]               # openings whose bottom row has every sibling
    bad[full[2 + variant], 0, 0, 3] ^= np.uint64(2)                # one limb of the first sibling of the leaf
    mine = np.array(leaves[idx.astype(np.int64)])
    top = M.climb(cr, mine, idx, bad, a, m) if M is MR else M.climb(cr, mine, idx, bad, a)
    ok = (top == nodes[-1]).all(axis=1).astype(np.uint8)
    assert ok.sum() == k - 1, "exactly the corrupted path fails"
    return mine, idx, paths, bad, np.array(nodes[-1]), ok


@functools.lru_cache(maxsize=None)
def data(case, variant=0):
    """(buffers: name -> (initial content, role), expected: name -> content of every out / inout buffer)"""
    f, cfg, cr = FP._config(case.label)
    t, r = cfg.t, cfg.rate
    s = dict(case.shape)
    e = case.entry
    seed = 0x57 + 1000 * variant + 7 * CASES.index(case)
    if e == "pmx_permute_batch_dev":
        st = synth.random_elements(f, s["n"] * t, seed=seed).reshape(s["n"], t, 4)
        bufs, want = {"d_states": (st, "inout")}, {"d_states": cr.permute_batch(st, threads=0)}
    elif e == "pmx_hash_batch_dev":
        n, in_len, out_len = s["n"], s["in_len"], s["out_len"]
        msgs = synth.random_elements(f, n * in_len, seed=seed).reshape(n, in_len, 4)
        bufs = {"d_in": (msgs, "in"), "d_out": (poison((n, out_len, 4), np.uint64, seed), "out")}
        want = {"d_out": cr.hash_batch(msgs, in_len, out_len, threads=0)}
    elif e == "pmx_sponge_absorb_batch_dev":
        n, in_len = s["n"], s["in_len"]
        st, tag, idx = _sponges(f, t, r, n, seed)
        msgs = synth.random_elements(f, n * in_len, seed=seed + 2).reshape(n, in_len, 4)
        bufs = {**_sponge_bufs(st, tag, idx), "d_in": (msgs, "in")}
        want = _absorbed(cr, st, tag, idx, msgs, np.arange(n + 1) * in_len)
    elif e == "pmx_sponge_squeeze_batch_dev":
        n, out_len = s["n"], s["out_len"]
        st, tag, idx = _sponges(f, t, r, n, seed)
        out, want = _squeezed(cr, st, tag, idx, out_len)
        bufs = {**_sponge_bufs(st, tag, idx), "d_out": (poison((n, out_len, 4), np.uint64, seed), "out")}
        want["d_out"] = out
    elif e == "pmx_sponge_absorb_varlen_batch_dev":
        n = s["n"]
        lens, offsets, elems, rows = FP._ragged(f, n, r, seed)           # lengths 0 .. 5 rate, empty rows among them
        assert lens.min() == 0 and lens.max() <= 5 * r            # (max_len = 5 rate is the caller's bound, not the longest row)
        st, tag, idx = _sponges(f, t, r, n, seed)
        bufs = {**_sponge_bufs(st, tag, idx), "d_in": (elems, "in"), "d_offsets": (offsets, "in")}
        want = _absorbed(cr, st, tag, idx, elems, offsets)
    elif e == "pmx_hash_varlen_batch_dev":
        n, out_len = s["n"], s["out_len"]
        lens, offsets, elems, rows = FP._ragged(f, n, r, seed)
        assert lens.min() == 0 and lens.max() <= 5 * r            # (max_len = 5 rate is the caller's bound, not the longest row)
        out = np.zeros((n, out_len, 4), dtype=np.uint64)
        for length in np.unique(lens):
            which = np.nonzero(lens == length)[0]
            msgs = np.stack([rows[i] for i in which]).reshape(len(which), int(length), 4)
            out[which] = cr.hash_batch(msgs, int(length), out_len, threads=0)
        bufs = {"d_in": (elems, "in"), "d_offsets": (offsets, "in"), "d_out": (poison(out.shape, np.uint64, seed), "out")}
        want = {"d_out": out}
    elif e in ("pmx_sponge_squeeze_bytes_batch_dev", "pmx_sponge_squeeze_bits_batch_dev"):
        n, length, bits = s["n"], s["length"], "bits" in e
        elems = SB._elems_for(length, SB._units(f.modulus)[1 if bits else 0])
        assert elems == 2 * r + 1
        st, tag, idx = _sponges(f, t, r, n, seed)
        el, want = _squeezed(cr, st, tag, idx, elems)
        bufs = {**_sponge_bufs(st, tag, idx), "d_out": (poison((n, length), np.uint8, seed), "out")}
        want["d_out"] = SB._cut(f.modulus, el, length, bits)
    elif e in ("pmx_merkle_2to1_dev", "pmx_merkle_ary_dev", "pmx_merkle_ragged_dev", "pmx_merkle_2to1_forest_dev", "pmx_merkle_ary_forest_dev"):
        a, n_trees = s.get("arity", 2), s.get("n_trees", 1)
        m = s.get("n_leaves") or n_trees * s["leaves_per_tree"]
        leaves = synth.random_elements(f, m, seed=seed)
        if "ragged" in e:
            nodes = MR.tree(cr, leaves, a)
        elif n_trees == 1 and a == 2:
            nodes = cr.merkle(leaves, threads=0)
        else:
            nodes = MA.forest(cr, leaves, n_trees, a)
        first = np.concatenate([leaves, poison((nodes.shape[0] - m, 4), np.uint64, seed)])      # the leaves in the first rows
        bufs, want = {"d_nodes": (first, "inout")}, {"d_nodes": nodes}
    elif e.endswith("verify_paths_dev"):
        M, a, _ = _tree_family(case)
        mine, idx, paths, bad, root, ok = _opening(case, seed, variant)
        k = s["k"]
        if e == "pmx_merkle_verify_paths_dev":
            bad = bad.reshape(k, -1, 4)                                  # [k][depth][4]
        bufs = {"d_leaves": (mine, "in"), "d_indices": (idx, "in"), "d_paths": (bad, "in"), "d_root": (root, "in"),
                "d_ok": (poison((k,), np.uint8, seed), "out"), "d_work": (poison((k, (a + 1) * 4), np.uint64, seed + 1), "scratch")}
        assert (ok.min(), ok.max()) == (0, 1)
        want = {"d_ok": ok}
    elif e.endswith("paths_dev"):
        M, a, _ = _tree_family(case)
        mine, idx, paths, bad, root, ok = _opening(case, seed, variant)
        nodes = M.cached_tree(case.label, a, s["n_leaves"])[1]
        bufs = {"d_nodes": (np.array(nodes), "in"), "d_indices": (idx, "in"), "d_paths": (poison(paths.shape, np.uint64, seed), "out")}
        want = {"d_paths": paths}
    elif e.endswith("update_dev"):
        M, a, _ = _tree_family(case)
        m, k = s["n_leaves"], s["k"]
        leaves, old = M.cached_tree(case.label, a, m)
        idx = _distinct(m, k, seed)
        new = synth.random_elements(f, k, seed=seed + 3)
        after = np.array(leaves)
        after[idx.astype(np.int64)] = new
        bufs = {"d_nodes": (np.array(old), "inout"), "d_indices": (idx, "in"), "d_new_leaves": (new, "in"),
                "d_work": (poison((k, (a + 1) * 4), np.uint64, seed), "scratch")}
        want = {"d_nodes": M.tree(cr, after, a)}
    else:
        raise KeyError(e)
    for name, (content, role) in bufs.items():
        assert content.flags["C_CONTIGUOUS"], name
        content.setflags(write=False)
    for name, content in want.items():
        assert bufs[name][1] in ("out", "inout") and content.nbytes == bufs[name][0].nbytes, name
        content.setflags(write=False)
    assert {n for n, (c, role) in bufs.items() if role in ("out", "inout")} == set(want)
    return bufs, want


# ---- the call ------------------------------------------------------------------------------------------------------------------------------
class Pointers:
    """name -> device address, with the ptr(name, shift) of the arenas that tests/test_gpu_footprint.py's dispatcher takes"""

    def __init__(self, tensors):
        self.tensors = tensors

    def ptr(self, name, shift=0):
        return self.tensors[name].data_ptr() + shift


def invoke(case, tensors, stream):
    """the call of the case on the device tensors `tensors`, on `stream` (a torch stream, which must be the current one); the status"""
    import torch
    assert torch.cuda.current_stream().cuda_stream == stream.cuda_stream
    s, e, p = dict(case.shape), case.entry, Pointers(tensors)
    if e in FP.ENTRIES:
        if e == "pmx_merkle_verify_paths_dev":
            s["depth"] = MA.shape(s["n_leaves"], 2)[0]
        if "varlen" in e:
            s["max_len"] = 5 * _rate(case.label)
        return FP._invoke(e, case.label, p, s)
    h, L, st = FP._config(case.label)[1].context()._h, _lib.lib(), stream.cuda_stream
    if e in ("pmx_sponge_squeeze_bytes_batch_dev", "pmx_sponge_squeeze_bits_batch_dev"):
        return getattr(L, e)(h, p.ptr("d_states"), p.ptr("d_mode_tag"), p.ptr("d_mode_index"), p.ptr("d_out"), s["length"], s["n"], st)
    a = s["arity"]
    if e in ("pmx_merkle_ary_dev", "pmx_merkle_ragged_dev"):
        return getattr(L, e)(h, p.ptr("d_nodes"), s["n_leaves"], a, st)
    if e == "pmx_merkle_ary_forest_dev":
        return L.pmx_merkle_ary_forest_dev(h, p.ptr("d_nodes"), s["n_trees"], s["leaves_per_tree"], a, st)
    if e in ("pmx_merkle_ary_paths_dev", "pmx_merkle_ragged_paths_dev"):
        return getattr(L, e)(h, p.ptr("d_nodes"), s["n_leaves"], a, p.ptr("d_indices"), s["k"], p.ptr("d_paths"), st)
    if e in ("pmx_merkle_ary_update_dev", "pmx_merkle_ragged_update_dev"):
        return getattr(L, e)(h, p.ptr("d_nodes"), s["n_leaves"], a, p.ptr("d_indices"), p.ptr("d_new_leaves"), s["k"], p.ptr("d_work"), st)
    depth = MR.shape(s["n_leaves"], a)[0]
    if e == "pmx_merkle_ary_verify_paths_dev":
        return L.pmx_merkle_ary_verify_paths_dev(h, p.ptr("d_leaves"), p.ptr("d_indices"), p.ptr("d_paths"), depth, a, s["k"], p.ptr("d_root"),
                                                 p.ptr("d_ok"), p.ptr("d_work"), st)
    if e == "pmx_merkle_ragged_verify_paths_dev":
        return L.pmx_merkle_ragged_verify_paths_dev(h, p.ptr("d_leaves"), p.ptr("d_indices"), p.ptr("d_paths"), depth, a, s["n_leaves"], s["k"],
                                                    p.ptr("d_root"), p.ptr("d_ok"), p.ptr("d_work"), st)
    raise KeyError(e)
