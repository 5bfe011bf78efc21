"""Matrix commitments on the device (pmx_matrix_leaves, pmx_matrix_commit, pmx_matrix_rows, pmx_matrix_verify_rows).  Everything is
bit-exact: no tolerance anywhere.

The oracle of the leaves is the C restatement (oracle/cref): CRef.hash_batch(rows [n][row_len][4], row_len, 1) on the row-major rows -
never the library under test.  The shapes are the smallest that have inactive lanes and a partial last workgroup (n_rows 1, 63, 64, 65,
257), exactly one, two and three absorb permutations (row_len 1, rate, rate + 1, 2 rate + 1) and n_rows != row_len in both orders, so a
kernel that swaps the two strides reads other elements (or leaves the matrix).  One oracle leg per config, shared by both layouts: about
3000 permutations.  The window engine of t = 3 starts above 32768 rows: there the column-major call is compared with pmx_hash_batch on
the row-major copy, code this family does not touch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sponge_amd as S
from sponge_amd import _lib, synth
from sponge_amd.merkle import MatrixCommitment, verify_rows

import arena
import merkle_ragged_oracle as M
from test_gpu_footprint import DeviceArena

pytestmark = pytest.mark.gpu

ROW, COL = _lib.MATRIX_ROW_MAJOR, _lib.MATRIX_COL_MAJOR
LAYOUTS = [ROW, COL]
ENGINE = {"t3": b"QuadEngine<5>", "t5": b"HybridEngine<5,5", "t9-bn254": b"HybridEngine<9,5", "lds-t16": b"LdsEngine<5>"}
N_ROWS = (1, 63, 64, 65, 257)
E = arena.E


def row_lens(rate):
    return (1, rate, rate + 1, 2 * rate + 1)


def engine_of(label, n, row_len):
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(M.config(label)[1].context(0)._h, _lib.OP_HASH, n, row_len, ctypes.byref(info)))
    return info


@functools.lru_cache(maxsize=None)
def rows_of(label, n_rows, row_len):
    """[n_rows][row_len][4], read-only: the matrix as rows"""
    rows = synth.random_elements(M.config(label)[0], n_rows * row_len, seed=0x3A7 + 1000 * n_rows + row_len).reshape(n_rows, row_len, 4)
    rows.setflags(write=False)
    return rows


def laid_out(rows, layout):
    """the flat matrix [n_rows * row_len][4] in the layout"""
    return np.ascontiguousarray(rows if layout == ROW else rows.transpose(1, 0, 2)).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def oracle_leaves(label, n_rows, row_len):
    out = M.config(label)[2].hash_batch(np.array(rows_of(label, n_rows, row_len)), row_len, 1, threads=0).reshape(n_rows, 4)
    out.setflags(write=False)
    return out


# ---- leaves against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=["row", "col"])
@pytest.mark.parametrize("label", sorted(ENGINE))
def test_leaves_against_the_oracle(label, layout):
    f, cfg, _ = M.config(label)
    ctx = cfg.context(0)
    for n_rows in N_ROWS:
        for row_len in row_lens(cfg.rate):
            assert engine_of(label, n_rows, row_len).engine.startswith(ENGINE[label])
            rows = rows_of(label, n_rows, row_len)
            got = ctx.matrix_leaves(laid_out(rows, layout), n_rows, row_len, layout)
            assert np.array_equal(got, oracle_leaves(label, n_rows, row_len)), (label, layout, n_rows, row_len)
    assert any(n < l for n in N_ROWS for l in row_lens(cfg.rate)) and any(n > l for n in N_ROWS for l in row_lens(cfg.rate))


def test_column_major_equals_row_major_on_the_t3_window_engine():
    """32769 rows of 3: above the quad engine's range.  The right-hand side is pmx_hash_batch on the transposed copy."""
    f, cfg, _ = M.config("t3")
    n_rows, row_len = 32769, 3
    assert engine_of("t3", n_rows, row_len).engine.startswith(b"HybridEngine<3,5")
    rows = synth.random_elements(f, n_rows * row_len, seed=0xC01).reshape(n_rows, row_len, 4)
    want = cfg.context(0).hash_batch(rows, row_len, 1).reshape(n_rows, 4)
    for layout in LAYOUTS:
        assert np.array_equal(cfg.context(0).matrix_leaves(laid_out(rows, layout), n_rows, row_len, layout), want), layout


# ---- the commitment ------------------------------------------------------------------------------------------------------------------
COMMITS = [("t3", 2, n) for n in (1, 2, 5, 64, 1000)] + [("t5", 4, 64), ("t5", 4, 70), ("t9-bn254", 8, 64), ("t9-bn254", 8, 100)]


@pytest.mark.parametrize("label,arity,n_rows", COMMITS)
def test_commit_is_the_ragged_tree_over_the_leaves(label, arity, n_rows):
    f, cfg, _ = M.config(label)
    ctx = cfg.context(0)
    assert arity == 2 or arity == cfg.rate
    row_len = cfg.rate + 1
    rows = synth.random_elements(f, n_rows * row_len, seed=0xC0 + n_rows).reshape(n_rows, row_len, 4)
    leaves = ctx.hash_batch(rows, row_len, 1).reshape(n_rows, 4)
    want_nodes, want_root = ctx.merkle_ragged(leaves, arity)
    assert want_nodes.shape[0] == M.shape(n_rows, arity)[1] and np.array_equal(want_nodes[:n_rows], leaves)
    for layout in LAYOUTS:
        flat = laid_out(rows, layout)
        nodes, root = ctx.matrix_commit(flat, n_rows, row_len, layout, arity)
        assert nodes.tobytes() == want_nodes.tobytes() and root.tobytes() == want_root.tobytes(), (label, arity, n_rows, layout)
        only_nodes, none = ctx.matrix_commit(flat, n_rows, row_len, layout, arity, want_root=False)       # root = NULL
        assert none is None and only_nodes.tobytes() == want_nodes.tobytes()
        none, only_root = ctx.matrix_commit(flat, n_rows, row_len, layout, arity, want_nodes=False)       # nodes = NULL
        assert none is None and only_root.tobytes() == want_root.tobytes()


def test_errors_that_need_the_context():
    f, cfg, _ = M.config("t3")
    lib, h = _lib.lib(), cfg.context(0)._h
    m = np.zeros((6, 4), dtype=np.uint64)
    out = np.full((16, 4), 0x33, dtype=np.uint64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert lib.pmx_matrix_commit(h, p(m), 2, 3, COL, 3, p(out), p(out)) == _lib.PMX_ERR_CONFIG and b"rate" in lib.pmx_last_error()
    idx, ok = np.zeros(2, dtype=np.uint64), np.full(2, 7, dtype=np.uint8)
    assert lib.pmx_matrix_verify_rows(h, p(m), 3, p(idx), p(out), 1, 3, 3, 2, p(out), p(ok)) == _lib.PMX_ERR_CONFIG
    assert (out == 0x33).all() and (ok == 7).all()
    assert lib.pmx_matrix_verify_rows(h, None, 3, None, None, 1, 2, 2, 0, p(out), None) == _lib.PMX_OK          # k = 0


# ---- slabs ---------------------------------------------------------------------------------------------------------------------------
def _bind(handle, name):
    fn = getattr(handle, name)
    fn.restype, fn.argtypes = (_lib.SIGNATURES.get(name) or _lib.TEST_HOOK_SIGNATURES[name])
    return fn


class HookLibrary:
    """libposeidon_mi355x_test.so bound next to whatever library the session uses, with a context of its own"""

    def __init__(self, cfg):
        self.handle = ctypes.CDLL(_lib.TEST_LIB_PATH)
        self.c = S.poseidon.c_config(cfg)
        self.ctx = ctypes.c_void_p()
        assert self.fn("pmx_ctx_create")(ctypes.byref(self.c), 0, ctypes.byref(self.ctx)) == _lib.PMX_OK

    def fn(self, name):
        return _bind(self.handle, name)

    def close(self):
        self.fn("pmx_test_matrix_slab_rows")(0)
        self.fn("pmx_ctx_destroy")(self.ctx)


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "page-locked"])
def test_slabs_give_the_bytes_of_one_slab(pinned):
    """200 x 5 column-major at t = 3 through slabs of 1, 7 and 64 rows (200, 29 and 4 slabs, the last one short: more slabs than the
    two buffers and than the context's events) against the one-slab call and the session library's"""
    f, cfg, _ = M.config("t3")
    n_rows, row_len, arity = 200, 5, 2
    rows = synth.random_elements(f, n_rows * row_len, seed=0x51AB).reshape(n_rows, row_len, 4)
    flat = laid_out(rows, COL)
    want_nodes, want_root = cfg.context(0).matrix_commit(flat, n_rows, row_len, COL, arity)
    hooks = HookLibrary(cfg)
    block = ctypes.c_void_p()
    try:
        src = ctypes.c_void_p(flat.ctypes.data)
        if pinned:
            assert hooks.fn("pmx_host_alloc")(ctypes.byref(block), flat.nbytes) == _lib.PMX_OK
            ctypes.memmove(block, src, flat.nbytes)
            src = block
        commit, leaves_fn, set_rows = hooks.fn("pmx_matrix_commit"), hooks.fn("pmx_matrix_leaves"), hooks.fn("pmx_test_matrix_slab_rows")
        for slab_rows in (0, 1, 7, 64):
            assert set_rows(slab_rows) == _lib.PMX_OK
            nodes, root = np.zeros_like(want_nodes), np.zeros(4, dtype=np.uint64)
            assert commit(hooks.ctx, src, n_rows, row_len, COL, arity, ctypes.c_void_p(nodes.ctypes.data), ctypes.c_void_p(root.ctypes.data)) == _lib.PMX_OK
            assert nodes.tobytes() == want_nodes.tobytes() and root.tobytes() == want_root.tobytes(), slab_rows
            leaves = np.zeros((n_rows, 4), dtype=np.uint64)
            assert leaves_fn(hooks.ctx, src, n_rows, row_len, COL, ctypes.c_void_p(leaves.ctypes.data)) == _lib.PMX_OK
            assert leaves.tobytes() == want_nodes[:n_rows].tobytes(), slab_rows
        rmajor = laid_out(rows, ROW)                          # and the row-major slabs (one contiguous copy each)
        assert set_rows(7) == _lib.PMX_OK
        assert leaves_fn(hooks.ctx, ctypes.c_void_p(rmajor.ctypes.data), n_rows, row_len, ROW, ctypes.c_void_p(leaves.ctypes.data)) == _lib.PMX_OK
        assert leaves.tobytes() == want_nodes[:n_rows].tobytes()
    finally:
        hooks.close()
        if block:
            hooks.fn("pmx_host_free")(block)
    assert np.array_equal(want_nodes[:n_rows], M.config("t3")[2].hash_batch(rows, row_len, 1, threads=0).reshape(n_rows, 4))   # 600 permutations


# ---- open and verify -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,arity,layout", [("t3", 2, "col"), ("t5", 4, "col"), ("t5", 4, "row")])
def test_open_then_verify_rows(label, arity, layout):
    f, cfg, _ = M.config(label)
    n_rows, row_len = 200, 2 * cfg.rate + 1
    rows = synth.random_elements(f, n_rows * row_len, seed=0x0FE).reshape(n_rows, row_len, 4)
    matrix = np.ascontiguousarray(rows.transpose(1, 0, 2)) if layout == "col" else rows
    com = MatrixCommitment(cfg, matrix, layout=layout, arity=arity)
    assert (com.n_rows, com.row_len) == (n_rows, row_len) and com.tree.n_leaves == n_rows
    assert np.array_equal(com.root, com.tree.nodes[-1])
    idx = np.array([0, 199, 64, 63, 150, 7, 199, 180], dtype=np.uint64)
    opened, paths = com.open(idx)
    assert np.array_equal(opened, rows[idx.astype(np.int64)])
    k = idx.shape[0]
    assert verify_rows(cfg, opened, idx, paths, com.root, n_rows, arity).all()
    flipped = opened.copy()
    flipped[2, row_len - 1, 3] ^= np.uint64(1)                # one limb of the LAST element of row 2
    assert verify_rows(cfg, flipped, idx, paths, com.root, n_rows, arity).tolist() == [i != 2 for i in range(k)]
    bad_paths = paths.copy()
    bad_paths.reshape(k, -1)[3, 5] ^= np.uint64(4)            # one limb of path 3 (its second sibling at the bottom level)
    assert verify_rows(cfg, opened, idx, bad_paths, com.root, n_rows, arity).tolist() == [i != 3 for i in range(k)]
    beyond = idx.copy()
    beyond[5] = n_rows                                        # an index that names no row; its digit at every level may still fit
    got = verify_rows(cfg, opened, beyond, paths, com.root, n_rows, arity)
    assert not got[5] and got[[0, 1, 2, 3, 4, 6, 7]].all()
    # a wrong n_rows of the same depth: only the rows at or beyond it fail (the root does not bind n_rows; the range test does)
    fewer = 170
    assert M.shape(fewer, arity)[0] == M.shape(n_rows, arity)[0]
    assert verify_rows(cfg, opened, idx, paths, com.root, fewer, arity).tolist() == [int(i) < fewer for i in idx]


# ---- the strided kernel's footprint --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", sorted(ENGINE))
def test_strided_kernel_footprint(label):
    """65 rows of rate + 1 elements through pmx_test_matrix_leaves_dev, matrix and digests carved out of one poisoned arena (tests/arena.py)
    at 16 mod 32: guard bands and the matrix intact, every digest the oracle's - under two different poison fills, so nothing outside the
    matrix went into a digest - on the carved layout and the control one, both layouts of the matrix."""
    f, cfg, _ = M.config(label)
    n_rows, row_len = 65, cfg.rate + 1
    info = engine_of(label, n_rows, row_len)
    assert info.engine.startswith(ENGINE[label]) and arena.span_fits(info.threads, cfg.t)
    rows = rows_of(label, n_rows, row_len)
    want = oracle_leaves(label, n_rows, row_len)
    hooks = HookLibrary(cfg)
    try:
        launch = hooks.fn("pmx_test_matrix_leaves_dev")
        stream = torch.cuda.current_stream().cuda_stream
        for layout in LAYOUTS:
            strides = (row_len, 1) if layout == ROW else (1, n_rows)
            for control in (False, True):
                for seed in (1, 2):
                    ar = DeviceArena([("d_matrix", n_rows * row_len * E, 16, "in"), ("d_leaves", n_rows * E, 16, "out")], seed=seed, control=control)
                    ar.put("d_matrix", laid_out(rows, layout))
                    ar.upload()
                    if not control and seed == 1:
                        for name in ("d_matrix", "d_leaves"):
                            shifted = {n: ar.ptr(n, 8 if n == name else 0) for n in ("d_matrix", "d_leaves")}
                            assert launch(hooks.ctx, shifted["d_matrix"], n_rows, row_len, *strides, shifted["d_leaves"], stream) == _lib.PMX_ERR_ARG
                            ar.unchanged()
                    assert launch(hooks.ctx, ar.ptr("d_matrix"), n_rows, row_len, *strides, ar.ptr("d_leaves"), stream) == _lib.PMX_OK
                    ar.finish()
                    assert np.array_equal(ar.get("d_leaves").reshape(n_rows, 4), want), (label, layout, control, seed)
    finally:
        hooks.close()


# ---- what was there stays what it was ------------------------------------------------------------------------------------------------
def test_existing_pins_again(golden):
    """pmx_hash_batch still gives the committed vectors, and PMX_OP_HASH still names the engines it named"""
    from gpu_helpers import ints, product_config
    g = golden("hash_merkle_vectors.json")
    for name in ("bls_t3_a5_8_31", "bn254_t9_a5_8_57"):
        cfg = product_config(name)
        for row in g[name]["hash"]:
            msg = cfg.field.from_ints(ints(row["in"])).reshape(1, row["L"], 4)
            assert cfg.field.to_ints(cfg.context().hash_batch(msg, row["L"], row["k"], n=1)) == ints(row["out"]), (name, row["L"], row["k"])
    for label, n, engine in (("t3", 32768, b"QuadEngine<5>"), ("t3", 32769, b"HybridEngine<3,5"), ("t9-bn254", 1000, b"HybridEngine<9,5"),
                             ("lds-t16", 1000, b"LdsEngine<5>")):
        info = engine_of(label, n, 3)
        assert info.engine.startswith(engine) and info.launches == 1 and info.width == M.config(label)[1].t, (label, n, info.engine)
