"""The device-resident matrix entries (include/poseidon_mi355x_resident.h: pmx_matrix_leaves_dev, pmx_matrix_commit_dev,
pmx_matrix_open_dev, pmx_matrix_verify_rows_dev) on the GPU.  Everything is bit-exact: no tolerance anywhere.

The oracle is the C restatement (oracle/cref): CRef.hash_batch on the row-major rows for the digests, tests/merkle_ragged_oracle.py for
the tree, the openings and the climb - never the library under test; the host entries of the family (pmx_matrix_commit, pmx_matrix_rows,
pmx_merkle_ragged_paths, pmx_matrix_verify_rows) are compared on top.  A matrix is laid into a buffer of exactly the view's extent whose
other elements hold a poison the oracle never sees, so a kernel that reads an element the view skips gives another digest.

Cells: quad-t3 (t = 3 up to 32768 rows), window-t3 (t = 3 above: one commit of 32768 + 5 rows and the stream / capture cases of the two
hashing entries; the verifier's hash of k <= 32768 rows is the quad engine's), t9-bn254 and lds-t16.  The engine of every hash launch is
asked of pmx_ctx_engine_info and asserted before the call.

One small case per entry and cell (65 rows of rate + 1 elements, column-major with ld = n_rows + 3, k = 9 queries that include 0,
n_rows - 1, a duplicate, n_rows and 2^63) carries the footprint, stream, capture and injected-failure tests; its expected buffers are
computed once and shared read-only."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sponge_amd import _lib, synth
from sponge_amd.merkle import DeviceMatrixCommitment, matrix_view_extent
from sponge_amd.poseidon import c_config, matrix_rows

import arena
import merkle_ragged_oracle as M
import test_gpu_footprint as FP
from test_gpu_footprint import DeviceArena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_CONFIG, ERR_HIP = _lib.PMX_OK, _lib.PMX_ERR_ARG, _lib.PMX_ERR_CONFIG, _lib.PMX_ERR_HIP
E = arena.E
LABELS = ["t3", "t9-bn254", "lds-t16"]                    # quad-t3, t9-bn254, lds-t16; window-t3 is t3 above 32768 rows
WINDOW_ROWS = 32768 + 5
N_ROWS = (1, 2, 5, 64, 65, 257)
ENTRIES = ("pmx_matrix_leaves_dev", "pmx_matrix_commit_dev", "pmx_matrix_open_dev", "pmx_matrix_verify_rows_dev")
MAX_UNITS = 0x7fffffff * 64                               # kMaxLaunchUnits
SLEEP_CYCLES = 50_000_000                                 # about 21 ms on the MI355X (tests/test_gpu_streams.py has the measurement)


def row_lens(rate):
    return (1, rate, rate + 1, 2 * rate + 1)


def arities(rate):
    return sorted({2, rate})


def views(n_rows, row_len):
    """name -> (row_stride, elem_stride)"""
    return {"row": (row_len, 1), "pitched": (row_len + 3, 1), "col": (1, n_rows), "col-ld": (1, n_rows + 3)}


def lay(rows, row_stride, elem_stride, seed=1):
    """the rows [n_rows][row_len][4] as a strided view of a buffer [extent][4] of poison"""
    n_rows, row_len = rows.shape[:2]
    extent = matrix_view_extent(n_rows, row_len, row_stride, elem_stride)
    assert extent == 1 + (n_rows - 1) * row_stride + (row_len - 1) * elem_stride
    flat = np.frombuffer(np.random.default_rng(0xBAD + seed).bytes(extent * E), dtype=np.uint64).reshape(extent, 4).copy()
    at = (np.arange(n_rows)[:, None] * row_stride + np.arange(row_len)[None, :] * elem_stride)
    assert np.unique(at).size == at.size
    flat[at.reshape(-1)] = rows.reshape(-1, 4)
    return flat


def ctx_of(label):
    return M.config(label)[1].context(0)


def assert_hash_engine(label, units, length):
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(ctx_of(label)._h, _lib.OP_HASH, units, length, ctypes.byref(info)))
    assert info.engine.startswith(FP._expected_engine(label, units)), (label, units, info.engine)
    assert arena.span_fits(info.threads, M.config(label)[1].t)
    return FP._cell(label, units)


@functools.lru_cache(maxsize=None)
def rows_of(label, n_rows, row_len, seed=0):
    rows = synth.random_elements(M.config(label)[0], n_rows * row_len, seed=0x5E5 + 1000 * n_rows + row_len + 77 * seed).reshape(n_rows, row_len, 4)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def oracle_nodes(label, n_rows, row_len, arity, seed=0):
    """the node array of the C port: the row digests, then the ragged tree over them"""
    cr = M.config(label)[2]
    leaves = cr.hash_batch(np.array(rows_of(label, n_rows, row_len, seed)), row_len, 1, threads=0).reshape(n_rows, 4)
    nodes = M.tree(cr, leaves, arity)
    assert nodes.shape[0] == M.shape(n_rows, arity)[1]
    nodes.setflags(write=False)
    return nodes


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to("cuda:0")


def down(t, dtype=np.uint64):
    return t.cpu().numpy().view(dtype)


def poison(nbytes, seed):
    return torch.from_numpy(np.frombuffer(np.random.default_rng(0xFACE + seed).bytes(max(nbytes, 1)), dtype=np.uint8).copy()).to("cuda:0")


def stream_now():
    return torch.cuda.current_stream().cuda_stream


# ---- leaves and commit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", LABELS)
def test_leaves_and_commit_of_every_view(label):
    f, cfg, cr = M.config(label)
    ctx, st = ctx_of(label), stream_now()
    cells = set()
    for n_rows in N_ROWS:
        for row_len in row_lens(cfg.rate):
            rows = rows_of(label, n_rows, row_len)
            host = {a: ctx.matrix_commit(np.array(rows).reshape(-1, 4), n_rows, row_len, _lib.MATRIX_ROW_MAJOR, a)[0] for a in arities(cfg.rate)}
            for name, (rs, es) in views(n_rows, row_len).items():
                d_matrix = up(lay(rows, rs, es))
                d_leaves = poison(n_rows * E, 1)
                cells.add(assert_hash_engine(label, n_rows, row_len))
                ctx.matrix_leaves_dev(d_matrix.data_ptr(), n_rows, row_len, rs, es, d_leaves.data_ptr(), st)
                torch.cuda.synchronize()
                want = oracle_nodes(label, n_rows, row_len, 2)
                assert down(d_leaves).tobytes() == want[:n_rows].tobytes(), (label, "leaves", n_rows, row_len, name)
                for a in arities(cfg.rate):
                    want = oracle_nodes(label, n_rows, row_len, a)
                    d_nodes = poison(want.nbytes, 2)
                    assert_hash_engine(label, n_rows, row_len)
                    ctx.matrix_commit_dev(d_matrix.data_ptr(), n_rows, row_len, rs, es, a, d_nodes.data_ptr(), st)
                    torch.cuda.synchronize()
                    got = down(d_nodes).tobytes()
                    assert got == want.tobytes(), (label, "commit against the oracle", n_rows, row_len, name, a)
                    assert got == host[a].tobytes(), (label, "commit against pmx_matrix_commit", n_rows, row_len, name, a)
    assert cells == {FP._cell(label, 1)}


def test_commit_on_the_t3_window_engine():
    """32768 + 5 rows of 3: above the quad engine's range, so the window engine hashes (and compresses level 1 on the quad kernels)"""
    label, n_rows, row_len, a = "t3", WINDOW_ROWS, 3, 2
    assert assert_hash_engine(label, n_rows, row_len) == "window-t3"
    rows, want = rows_of(label, n_rows, row_len), oracle_nodes(label, n_rows, row_len, a)
    ctx = ctx_of(label)
    host, _ = ctx.matrix_commit(np.ascontiguousarray(rows.transpose(1, 0, 2)).reshape(-1, 4), n_rows, row_len, _lib.MATRIX_COL_MAJOR, a)
    for name in ("col-ld", "pitched"):
        rs, es = views(n_rows, row_len)[name]
        d_matrix, d_nodes = up(lay(rows, rs, es)), poison(want.nbytes, 3)
        ctx.matrix_commit_dev(d_matrix.data_ptr(), n_rows, row_len, rs, es, a, d_nodes.data_ptr(), stream_now())
        torch.cuda.synchronize()
        got = down(d_nodes).tobytes()
        assert got == want.tobytes() and got == host.tobytes(), name


# ---- the shared small case of every entry -----------------------------------------------------------------------------------------------
CASE_ROWS, CASE_K = 65, 9


def case_shape(label, window=False):
    rate = M.config(label)[1].rate
    n_rows, row_len = (WINDOW_ROWS, 3) if window else (CASE_ROWS, rate + 1)
    arity = 2 if label == "t3" else rate
    return dict(n_rows=n_rows, row_len=row_len, row_stride=1, elem_stride=n_rows + 3, arity=arity, k=CASE_K, depth=M.shape(n_rows, arity)[0])


def case_indices(n_rows, variant):
    """0, n_rows - 1, a duplicate, n_rows and 2^63 among the k; other values and another order for variant 1"""
    idx = [0, n_rows - 1, 7, 7, n_rows, 1 << 63, 33, n_rows - 2, 1]
    if variant:
        idx = [n_rows - 1, 5, 1 << 63, 0, 40, 40, n_rows, 2, n_rows - 3]
    return np.array(idx, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def case_data(entry, label, variant=0, window=False):
    """(shape, buffers: name -> (initial content, align, role), expected: name -> content of every out buffer), arrays read-only"""
    f, cfg, cr = M.config(label)
    s = case_shape(label, window)
    n, L, a, k, depth = s["n_rows"], s["row_len"], s["arity"], s["k"], s["depth"]
    rows, nodes = rows_of(label, n, L, variant), oracle_nodes(label, n, L, a, variant)
    flat = lay(rows, s["row_stride"], s["elem_stride"], seed=5 + variant)
    idx = case_indices(n, variant)
    valid = idx < np.uint64(n)
    opened = np.zeros((k, L, 4), dtype=np.uint64)
    opened[valid] = rows[idx[valid].astype(np.int64)]
    paths = np.zeros((k, depth, a - 1, 4), dtype=np.uint64)
    paths[valid] = M.open_paths(nodes, n, a, idx[valid])
    junk = lambda shape, dtype, seed: np.frombuffer(np.random.default_rng(0xD00D + seed + variant).bytes(int(np.prod(shape)) * np.dtype(dtype).itemsize),
                                                    dtype=dtype).reshape(shape).copy()
    if entry == "pmx_matrix_leaves_dev":
        bufs = {"d_matrix": (flat, 16, "in"), "d_leaves": (junk((n, 4), np.uint64, 1), 16, "out")}
        want = {"d_leaves": np.array(nodes[:n])}
    elif entry == "pmx_matrix_commit_dev":
        bufs = {"d_matrix": (flat, 16, "in"), "d_nodes": (junk(nodes.shape, np.uint64, 2), 16, "out")}
        want = {"d_nodes": np.array(nodes)}
    elif entry == "pmx_matrix_open_dev":
        bufs = {"d_matrix": (flat, 16, "in"), "d_nodes": (np.array(nodes), 16, "in"), "d_indices": (idx, 8, "in"),
                "d_rows": (junk(opened.shape, np.uint64, 3), 16, "out"), "d_paths": (junk(paths.shape, np.uint64, 4), 16, "out")}
        want = {"d_rows": opened, "d_paths": paths}
    elif entry == "pmx_matrix_verify_rows_dev":
        # true openings, one limb of the LAST element of row 2 flipped, one limb of path 6 flipped, two indices that name no row
        bad_rows, bad_paths = opened.copy(), paths.copy()
        bad_rows[2 + variant, L - 1, 3] ^= np.uint64(1)
        bad_paths[6 + variant, depth - 1, 0, 1] ^= np.uint64(4)
        ok = np.zeros(k, dtype=np.uint8)
        where = np.nonzero(valid)[0]
        digests = cr.hash_batch(bad_rows[where], L, 1, threads=0).reshape(-1, 4)
        top = M.climb(cr, digests, idx[where], bad_paths[where], a, n)
        ok[where] = (top == nodes[-1]).all(axis=1)
        assert ok.sum() == valid.sum() - 2 and not ok[2 + variant] and not ok[6 + variant] and valid[2 + variant] and valid[6 + variant]
        bufs = {"d_rows": (bad_rows, 16, "in"), "d_indices": (idx, 8, "in"), "d_paths": (bad_paths, 16, "in"), "d_root": (np.array(nodes[-1]), 16, "in"),
                "d_ok": (junk((k,), np.uint8, 5), 1, "out"), "d_work": (junk((k, (a + 2) * 4), np.uint64, 6), 16, "scratch")}
        want = {"d_ok": ok}
    else:
        raise KeyError(entry)
    for content in [c for c, _, _ in bufs.values()] + list(want.values()):
        assert content.flags["C_CONTIGUOUS"]
        content.setflags(write=False)
    return s, bufs, want


def invoke(fn, h, entry, s, p, stream, null=()):
    """the call of `entry`; p(name) is a buffer's device address, `null` names the pointers passed as NULL"""
    q = lambda name: None if name in null else p(name)
    view = (s["n_rows"], s["row_len"], s["row_stride"], s["elem_stride"])
    if entry == "pmx_matrix_leaves_dev":
        return fn(entry)(h, q("d_matrix"), *view, q("d_leaves"), stream)
    if entry == "pmx_matrix_commit_dev":
        return fn(entry)(h, q("d_matrix"), *view, s["arity"], q("d_nodes"), stream)
    if entry == "pmx_matrix_open_dev":
        return fn(entry)(h, q("d_matrix"), *view, q("d_nodes"), s["arity"], q("d_indices"), s["k"], q("d_rows"), q("d_paths"), stream)
    if entry == "pmx_matrix_verify_rows_dev":
        return fn(entry)(h, q("d_rows"), s["row_len"], q("d_indices"), q("d_paths"), s["depth"], s["arity"], s["n_rows"], s["k"], q("d_root"),
                         q("d_ok"), q("d_work"), stream)
    raise KeyError(entry)


def session_fn(name):
    return getattr(_lib.lib(), name)


def assert_case_engine(entry, label, s):
    if entry == "pmx_matrix_open_dev":
        return None                                       # two gathers: no permutation engine
    units = s["k"] if entry == "pmx_matrix_verify_rows_dev" else s["n_rows"]
    return assert_hash_engine(label, units, s["row_len"])


def arena_of(bufs, seed, control):
    a = DeviceArena([(name, content.nbytes, align, role) for name, (content, align, role) in bufs.items()], seed=seed, control=control)
    for name, (content, align, role) in bufs.items():
        if role != "out":                                 # an out buffer keeps the arena's poison
            a.put(name, content)
    return a.upload()


def assert_exact(a, want, what):
    for name, content in want.items():
        assert a.get(name, np.uint8).tobytes() == content.tobytes(), (what, name)


# ---- open -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", LABELS)
def test_open_against_the_host_entries(label):
    f, cfg, cr = M.config(label)
    ctx, st, L = ctx_of(label), stream_now(), _lib.lib()
    n_rows, row_len = 65, cfg.rate + 1
    rows = rows_of(label, n_rows, row_len)
    idx = case_indices(n_rows, 0)
    valid = idx < np.uint64(n_rows)
    k = idx.shape[0]
    d_idx = up(idx)
    host_rows = matrix_rows(np.array(rows).reshape(-1, 4), n_rows, row_len, _lib.MATRIX_ROW_MAJOR, idx[valid])
    for a in arities(cfg.rate):
        nodes = oracle_nodes(label, n_rows, row_len, a)
        depth = M.shape(n_rows, a)[0]
        host_paths = np.zeros((int(valid.sum()), depth, a - 1, 4), dtype=np.uint64)
        good = np.ascontiguousarray(idx[valid])
        _lib.check(L.pmx_merkle_ragged_paths(ctypes.c_void_p(nodes.ctypes.data), n_rows, a, ctypes.c_void_p(good.ctypes.data), good.shape[0],
                                             ctypes.c_void_p(host_paths.ctypes.data)))
        assert np.array_equal(host_paths, M.open_paths(nodes, n_rows, a, good))
        d_nodes = up(nodes)
        for name, (rs, es) in views(n_rows, row_len).items():
            d_matrix = up(lay(rows, rs, es))
            d_rows, d_paths = poison(k * row_len * E, 7), poison(k * depth * (a - 1) * E, 8)
            ctx.matrix_open_dev(d_matrix.data_ptr(), n_rows, row_len, rs, es, d_nodes.data_ptr(), a, d_idx.data_ptr(), k, d_rows.data_ptr(),
                                d_paths.data_ptr(), st)
            torch.cuda.synchronize()
            got_rows, got_paths = down(d_rows).reshape(k, row_len, 4), down(d_paths).reshape(k, depth, a - 1, 4)
            assert np.array_equal(got_rows[valid], host_rows) and np.array_equal(got_paths[valid], host_paths), (label, a, name)
            assert not got_rows[~valid].any() and not got_paths[~valid].any(), (label, a, name, "an index that names no row must give zeros")
            # d_nodes = NULL: the rows alone, whatever the arity says
            d_rows2, before = poison(k * row_len * E, 9), d_paths.clone()
            ctx.matrix_open_dev(d_matrix.data_ptr(), n_rows, row_len, rs, es, None, 0, d_idx.data_ptr(), k, d_rows2.data_ptr(), None, st)
            torch.cuda.synchronize()
            assert torch.equal(d_rows2, d_rows) and torch.equal(before, d_paths)
    # one row: the leaf is the root, a path has no level
    one = rows_of(label, 1, row_len)
    d_matrix, d_nodes, d_rows = up(one), poison(E, 10), poison(k * row_len * E, 11)
    ctx.matrix_commit_dev(d_matrix.data_ptr(), 1, row_len, row_len, 1, 2, d_nodes.data_ptr(), st)
    ctx.matrix_open_dev(d_matrix.data_ptr(), 1, row_len, row_len, 1, d_nodes.data_ptr(), 2, d_idx.data_ptr(), k, d_rows.data_ptr(), None, st)
    torch.cuda.synchronize()
    assert down(d_nodes).tobytes() == oracle_nodes(label, 1, row_len, 2).tobytes()
    got = down(d_rows).reshape(k, row_len, 4)
    assert all((got[i] == one[0]).all() if idx[i] == 0 else not got[i].any() for i in range(k))


# ---- verify -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", LABELS)
def test_verify_rows_verdicts(label):
    """true openings, a flipped limb in a row, a flipped limb in a path, an index >= n_rows, a wrong root: the C port's verdicts and those
    of pmx_matrix_verify_rows"""
    ctx, st = ctx_of(label), stream_now()
    s, bufs, want = case_data("pmx_matrix_verify_rows_dev", label)
    k, a, n = s["k"], s["arity"], s["n_rows"]
    _, open_bufs, open_want = case_data("pmx_matrix_open_dev", label)
    idx = bufs["d_indices"][0]
    valid = idx < np.uint64(n)

    def verdicts(rows, indices, paths, root):
        dev = {name: up(x) for name, x in (("rows", rows), ("idx", indices), ("paths", paths), ("root", root))}
        d_ok, d_work = poison(k, 12), poison(k * (a + 2) * E, 13)
        assert assert_hash_engine(label, k, s["row_len"]) == FP._cell(label, k)
        ctx.matrix_verify_rows_dev(dev["rows"].data_ptr(), s["row_len"], dev["idx"].data_ptr(), dev["paths"].data_ptr(), s["depth"], a, n, k,
                                   dev["root"].data_ptr(), d_ok.data_ptr(), d_work.data_ptr(), st)
        torch.cuda.synchronize()
        got = down(d_ok, np.uint8)
        host = ctx.matrix_verify_rows(np.array(rows), np.array(indices), np.array(paths), s["depth"], a, n, np.array(root))
        assert np.array_equal(got, host), (label, "the verdicts of pmx_matrix_verify_rows", got, host)
        return got

    root = bufs["d_root"][0]
    assert np.array_equal(verdicts(open_want["d_rows"], idx, open_want["d_paths"], root), valid.astype(np.uint8))       # true openings
    assert np.array_equal(verdicts(bufs["d_rows"][0], idx, bufs["d_paths"][0], root), want["d_ok"])                    # the two flips
    moved = idx.copy()
    moved[0] = n                                          # a true opening under an index that names no row (its digits may still fit)
    assert np.array_equal(verdicts(open_want["d_rows"], moved, open_want["d_paths"], root), (valid & (np.arange(k) != 0)).astype(np.uint8))
    wrong = root.copy()
    wrong[0] ^= np.uint64(1)
    assert not verdicts(open_want["d_rows"], idx, open_want["d_paths"], wrong).any()


# ---- footprint --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", LABELS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_footprint_in_a_guarded_arena(entry, label):
    """every buffer of the call out of one poisoned arena, at base + 16 * odd (8 * odd, odd) and again at base + 256 k, under two
    poison fills: guards, inputs and the unwritten ranges unchanged, every out buffer the C port's"""
    s, bufs, want = case_data(entry, label)
    h = ctx_of(label)._h
    for control in (False, True):
        for seed in (1, 2):
            a = arena_of(bufs, seed, control)
            assert_case_engine(entry, label, s)
            assert invoke(session_fn, h, entry, s, a.ptr, stream_now()) == OK, _lib.lib().pmx_last_error()
            a.finish()
            assert_exact(a, want, (entry, label, control, seed))
    if entry == "pmx_matrix_open_dev":                    # rows only: d_nodes and d_paths are not touched
        a = arena_of(bufs, 3, False)
        assert invoke(session_fn, h, entry, s, a.ptr, stream_now(), null=("d_nodes", "d_paths")) == OK
        a.finish(written={"d_paths": (0, 0)})
        assert_exact(a, {"d_rows": want["d_rows"]}, (entry, label, "rows only"))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_arena_unchanged():
    """one call per error of the header; each is refused before anything is launched"""
    label = "t3"
    h, L = ctx_of(label)._h, _lib.lib()
    element_arrays = {"pmx_matrix_leaves_dev": ("d_matrix", "d_leaves"), "pmx_matrix_commit_dev": ("d_matrix", "d_nodes"),
                      "pmx_matrix_open_dev": ("d_matrix", "d_nodes", "d_rows", "d_paths"),
                      "pmx_matrix_verify_rows_dev": ("d_rows", "d_paths", "d_root", "d_work")}
    for entry in ENTRIES:
        s, bufs, want = case_data(entry, label)
        a = arena_of(bufs, 4, False)
        cases = []                                        # (shape overrides, null pointers, shifts, status, needle)
        for name in bufs:
            if not (entry == "pmx_matrix_open_dev" and name in ("d_nodes", "d_paths")):
                cases.append(({}, (name,), {}, ERR_ARG, b"null pointer"))
        if entry == "pmx_matrix_open_dev":
            cases += [({}, ("d_nodes",), {}, ERR_ARG, b"d_paths without d_nodes"), ({}, ("d_paths",), {}, ERR_ARG, b"d_nodes without d_paths")]
        if "d_matrix" in bufs:
            cases += [({"n_rows": 0}, (), {}, ERR_ARG, b"at least one row"), ({"row_len": 0}, (), {}, ERR_ARG, b"at least one element"),
                      ({"row_stride": 0}, (), {}, ERR_ARG, b"stride"), ({"elem_stride": 0}, (), {}, ERR_ARG, b"stride"),
                      ({"elem_stride": 1 << 59}, (), {}, ERR_ARG, b"overflows"),
                      ({"n_rows": MAX_UNITS + 1, "row_len": 1, "row_stride": 1, "elem_stride": 1}, (), {}, ERR_ARG, b"batch too large")]
        else:
            cases += [({"row_len": 0}, (), {}, ERR_ARG, b"at least one element"), ({"n_rows": 0}, (), {}, ERR_ARG, b"at least one leaf"),
                      ({"depth": s["depth"] + 1}, (), {}, ERR_ARG, b"is not the depth"), ({"depth": 0}, (), {}, ERR_ARG, b"is not the depth"),
                      ({"k": MAX_UNITS // 2 + 1}, (), {}, ERR_ARG, b"batch too large")]
        if entry == "pmx_matrix_open_dev":
            cases += [({"k": MAX_UNITS // s["row_len"] + 1}, (), {}, ERR_ARG, b"batch too large")]
        if entry != "pmx_matrix_leaves_dev":
            cases += [({"arity": 1}, (), {}, ERR_ARG, b"arity must be at least 2"), ({"arity": 0}, (), {}, ERR_ARG, b"arity must be at least 2"),
                      ({"arity": 3}, (), {}, ERR_CONFIG, b"exceeds the rate")]
        for name in element_arrays[entry]:
            cases.append(({}, (), {name: 8}, ERR_ARG, b"device pointers must be 16-byte aligned"))
        if "d_indices" in bufs:
            cases.append(({}, (), {"d_indices": 4}, ERR_ARG, b"d_indices must be 8-byte aligned"))
        for over, null, shift, status, needle in cases:
            shape = dict(s, **over)
            if "arity" in over and "depth" in s and over["arity"] == 3:
                shape["depth"] = M.shape(s["n_rows"], 3)[0]
            rc = invoke(session_fn, h, entry, shape, lambda name: a.ptr(name, shift.get(name, 0)), stream_now(), null=null)
            assert rc == status and needle in L.pmx_last_error(), (entry, over, null, shift, rc, L.pmx_last_error())
            a.unchanged()
        if "d_indices" in bufs:                           # k = 0: PMX_OK, nothing launched, the arrays indexed by k may be NULL
            by_k = ("d_indices", "d_rows", "d_paths", "d_ok", "d_work")
            assert invoke(session_fn, h, entry, dict(s, k=0), a.ptr, stream_now(), null=by_k) == OK
            a.unchanged()


# ---- streams and capture ----------------------------------------------------------------------------------------------------------------
STREAM_CASES = [(entry, label, False) for entry in ENTRIES for label in LABELS] + [(entry, "t3", True) for entry in ENTRIES[:2]]
STREAM_IDS = [f"{e[4:]}-{'window-t3' if w else FP._cell(l, 1)}" for e, l, w in STREAM_CASES]


@pytest.fixture(scope="module")
def side():
    s = torch.cuda.Stream(device="cuda:0")
    yield s
    s.synchronize()


def test_the_stream_cases_cover_the_four_cells():
    cells = {}
    for entry, label, window in STREAM_CASES:
        cell = assert_case_engine(entry, label, case_data(entry, label, 0, window)[0])
        cells.setdefault(entry, set()).add(cell)
    small = {"quad-t3", "t9-bn254", "lds-t16"}
    assert cells["pmx_matrix_leaves_dev"] == cells["pmx_matrix_commit_dev"] == small | {"window-t3"}
    assert cells["pmx_matrix_verify_rows_dev"] == small and cells["pmx_matrix_open_dev"] == {None}


@pytest.mark.parametrize("entry,label,window", STREAM_CASES, ids=STREAM_IDS)
def test_ordered_on_a_side_stream(entry, label, window, side):
    """the buffers the call reads hold poison; behind a delay on a non-blocking side stream the inputs arrive by device-to-device copies,
    the call follows, the outputs are copied out - no host synchronisation in between.  The delay must still be pending when the call
    returns (else the run is inconclusive and FAILS).  The identical call ran once before on throw-away buffers."""
    s, bufs, want = case_data(entry, label, 0, window)
    assert_case_engine(entry, label, s)
    h = ctx_of(label)._h
    reads = [n for n, (c, al, role) in bufs.items() if role == "in"]
    staging = {n: up(bufs[n][0]) for n in reads}
    dev = {n: poison(c.nbytes, 20 + i) for i, (n, (c, al, role)) in enumerate(bufs.items())}
    spare = {n: (staging[n].clone() if n in staging else poison(c.nbytes, 40 + i)) for i, (n, (c, al, role)) in enumerate(bufs.items())}
    result = {n: torch.empty_like(dev[n]) for n in want}
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert invoke(session_fn, h, entry, s, lambda n: spare[n].data_ptr(), side.cuda_stream) == OK
        side.synchronize()
        torch.cuda.synchronize()
        torch.cuda._sleep(SLEEP_CYCLES)
        e_delay = torch.cuda.Event()
        e_delay.record(side)
        for n in reads:
            dev[n].copy_(staging[n], non_blocking=True)
        rc = invoke(session_fn, h, entry, s, lambda n: dev[n].data_ptr(), side.cuda_stream)
        delay_over = e_delay.query()
        for n in want:
            result[n].copy_(dev[n], non_blocking=True)
    side.synchronize()
    assert rc == OK, _lib.lib().pmx_last_error()
    if delay_over:
        pytest.fail("delay too short: inconclusive")
    for n in want:
        assert down(result[n], np.uint8).tobytes() == want[n].tobytes(), (entry, label, n)
    torch.cuda.synchronize()
    for n in want:
        assert torch.equal(result[n], dev[n]), (entry, label, n, "changed after the copy-out")


@pytest.mark.parametrize("entry,label,window", STREAM_CASES, ids=STREAM_IDS)
def test_captured_into_a_graph(entry, label, window, side):
    """one call captured on the side stream: capturing executes nothing, the replay gives the C port's answer for input set A, and - the
    same buffers overwritten in place with set B - for B"""
    s, bufs, want = case_data(entry, label, 0, window)
    assert_case_engine(entry, label, s)
    h = ctx_of(label)._h
    dev = {n: up(c) for n, (c, al, role) in bufs.items()}
    torch.cuda.synchronize()
    before = {n: t.clone() for n, t in dev.items()}
    g, rc = torch.cuda.CUDAGraph(), None
    try:
        with torch.cuda.graph(g, stream=side, capture_error_mode="global"):
            rc = invoke(session_fn, h, entry, s, lambda n: dev[n].data_ptr(), torch.cuda.current_stream().cuda_stream)
    except RuntimeError as exc:
        pytest.fail(f"{entry} [{label}]: the capture failed (status {rc}, {_lib.lib().pmx_last_error()}): {exc}")
    assert rc == OK, _lib.lib().pmx_last_error()
    torch.cuda.synchronize()
    for n in dev:
        assert torch.equal(before[n], dev[n]), (entry, label, n, "capturing executed something")
    g.replay()
    torch.cuda.synchronize()
    for n in want:
        assert down(dev[n], np.uint8).tobytes() == want[n].tobytes(), (entry, label, n, "replay on input set A")
    if window:
        return                                            # the large case is replayed once
    s_b, bufs_b, want_b = case_data(entry, label, 1, window)
    assert s_b == s and all(not np.array_equal(bufs[n][0], bufs_b[n][0]) for n in bufs), "input set B must differ from A"
    for n, (c, al, role) in bufs_b.items():
        dev[n].copy_(up(c))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for n in want_b:
        assert down(dev[n], np.uint8).tobytes() == want_b[n].tobytes(), (entry, label, n, "replay on input set B")


def test_cold_chain_capture_in_a_fresh_process(tmp_path):
    """commit, open and verify captured as ONE graph in a child process whose first launch of any kernel of the library is the captured
    one (tests/matrix_resident_cold_worker.py).  The parent leaves the inputs and the C port's answers as .npy files."""
    label = "t3"
    s, bufs, want = case_data("pmx_matrix_open_dev", label)
    ok = (bufs["d_indices"][0] < np.uint64(s["n_rows"])).astype(np.uint8)
    np.save(tmp_path / "matrix.npy", bufs["d_matrix"][0])
    np.save(tmp_path / "indices.npy", bufs["d_indices"][0])
    np.save(tmp_path / "nodes.npy", bufs["d_nodes"][0])
    np.save(tmp_path / "rows.npy", want["d_rows"])
    np.save(tmp_path / "paths.npy", want["d_paths"])
    np.save(tmp_path / "ok.npy", ok)
    np.save(tmp_path / "shape.npy", np.array([s[x] for x in ("n_rows", "row_len", "row_stride", "elem_stride", "arity", "k")], dtype=np.int64))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "matrix_resident_cold_worker.py"), str(tmp_path)], capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0 and "cold chain ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- the Python class -------------------------------------------------------------------------------------------------------------------
def test_device_matrix_commitment_runs_the_chain_on_device_pointers():
    label = "t9-bn254"
    s, bufs, want = case_data("pmx_matrix_open_dev", label)
    cfg = M.config(label)[1]
    d_matrix, d_idx, d_ok = up(bufs["d_matrix"][0]), up(bufs["d_indices"][0]), poison(s["k"], 14)
    with DeviceMatrixCommitment(cfg, d_matrix.data_ptr(), s["n_rows"], s["row_len"], s["row_stride"], s["elem_stride"], s["arity"],
                                stream=stream_now()) as com:
        assert (com.depth, com.n_nodes) == M.shape(s["n_rows"], s["arity"]) and com.extent * E == d_matrix.numel()
        d_rows, d_paths = com.open(d_idx.data_ptr(), s["k"])
        com.verify_rows_dev(d_rows, d_idx.data_ptr(), d_paths, s["k"], d_ok.data_ptr())
        torch.cuda.synchronize()
        root, rows, paths = (np.zeros(shape, dtype=np.uint64) for shape in ((4,), want["d_rows"].shape, want["d_paths"].shape))
        for host, ptr in ((root, com.root_ptr), (rows, d_rows), (paths, d_paths)):
            _lib.check(_lib.lib().pmx_device_download(0, ctypes.c_void_p(host.ctypes.data), ptr, host.nbytes, None))
        _lib.check(_lib.lib().pmx_stream_synchronize(0, None))
        assert np.array_equal(root, bufs["d_nodes"][0][-1]) and np.array_equal(rows, want["d_rows"]) and np.array_equal(paths, want["d_paths"])
        assert np.array_equal(down(d_ok, np.uint8), (bufs["d_indices"][0] < np.uint64(s["n_rows"])).astype(np.uint8))
        only_rows, none = com.open(d_idx.data_ptr(), s["k"], with_paths=False)
        assert none is None


# ---- injected HIP failures --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _test_library():
    return ctypes.CDLL(_lib.TEST_LIB_PATH)


def hook_fn(name):
    fn = getattr(_test_library(), name)
    fn.restype, fn.argtypes = _lib.SIGNATURES.get(name) or _lib.RESIDENT_SIGNATURES.get(name) or _lib.TEST_HOOK_SIGNATURES[name]
    return fn


@pytest.mark.parametrize("label", ["t3", "t9-bn254"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_every_checked_hip_call_failed_once(entry, label):
    """the test library fails the k-th checked HIP call for every k the call makes: PMX_ERR_HIP in the injector's words, guards and inputs
    unchanged, nothing in flight, and the same call repeated is exact.  An injected failure is a return value made on the host: nothing
    reaches the device that a clean call would not send."""
    s, bufs, want = case_data(entry, label)
    c, h = c_config(M.config(label)[1]), ctypes.c_void_p()
    assert hook_fn("pmx_ctx_create")(ctypes.byref(c), 0, ctypes.byref(h)) == OK
    last = lambda: hook_fn("pmx_last_error")() or b""
    try:
        a = arena_of(bufs, 6, False)
        assert hook_fn("pmx_test_fail_hip")(1 << 40) == OK                        # a count no call reaches: the call's own K
        rc = invoke(hook_fn, h, entry, s, a.ptr, stream_now())
        K = hook_fn("pmx_test_hip_calls")()
        assert hook_fn("pmx_test_fail_hip")(0) == OK
        assert rc == OK, last()
        a.finish()
        assert_exact(a, want, (entry, label, "clean"))
        launches = {"pmx_matrix_leaves_dev": 1, "pmx_matrix_commit_dev": 1 + s["depth"], "pmx_matrix_open_dev": 2,
                    "pmx_matrix_verify_rows_dev": 3 + 2 * s["depth"]}[entry]       # (the verifier: hash, copy, two per level, verdicts)
        assert K == launches, (entry, label, K)
        print(f"{entry} [{label}]: {K} checked HIP calls")
        for k in range(1, K + 1):
            a = arena_of(bufs, 6 + k, False)
            assert hook_fn("pmx_test_fail_hip")(k) == OK
            rc = invoke(hook_fn, h, entry, s, a.ptr, stream_now())
            fired = hook_fn("pmx_test_hip_fired")() or b""
            assert hook_fn("pmx_test_fail_hip")(0) == OK
            if rc == ERR_HIP and b"injected" not in last():
                pytest.exit(f"{entry} [{label}] k={k}: PMX_ERR_HIP: {last()}", returncode=3)
            assert rc == ERR_HIP and b"injected in place of" in last() and fired.startswith(b"injected in place of"), (entry, k, rc, last())
            assert hook_fn("pmx_stream_synchronize")(0, None) == OK, last()     # nothing in flight
            a.finish()                                                            # guards and inputs as they were
            rc = invoke(hook_fn, h, entry, s, a.ptr, stream_now())               # the same call again, unarmed
            assert rc == OK, (entry, k, last())
            a.finish()
            assert_exact(a, want, (entry, label, k, "repeated"))
    finally:
        hook_fn("pmx_test_fail_hip")(0)
        assert hook_fn("pmx_ctx_destroy")(h) == OK
