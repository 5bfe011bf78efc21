"""The device staging of the host-buffer entries across calls (sponge_amd/csrc/pmx_ctx.hpp: HostCall; pmx_staging.hpp): the four
grow-only blocks of a context persist from call to call, so every test here runs on ONE context per config, made by pmx_ctx_create so
that no earlier test has grown its blocks.  Results against the C port (oracle/cref).  Configs: t = 3 at rate 2 and t = 9 at rate 8.
- Grow and return: every host-buffer entry at its smallest shape, at a shape that grows every block it uses (the sponge entries cross
  from the packed to the resident path), at the small shape again, then a different entry; the entries in two orders.
- The mode words on both sides of their padding to 16 bytes: n = 1, 3, 4, 5 sponges.
- The packed limit: the largest n whose packed size is at most 64 KiB, and one more.
- Verifiers whose `ok` section is ragged: k = 1 and k = 5, one path wrong.
(Fixed-depth walks of several pieces: tests/test_gpu_merkle_fixed.py, through the test library's piece hook.)"""
import ctypes

import numpy as np
import pytest

import sponge_amd as S
from sponge_amd import _lib, synth
from sponge_amd.poseidon import Context, _ptr, c_config

import merkle_ary_oracle as M
import merkle_fixed_oracle as F
import merkle_ragged_oracle as R

pytestmark = pytest.mark.gpu

LABELS = {"t3": 2, "t9-bn254": 4}      # label: the arity of its trees
SMALL_CALL_BYTES = 64 * 1024           # kSmallCallBytes (pmx_ctx.hpp)


@pytest.fixture(scope="module", params=list(LABELS))
def box(request):
    """(label, field, config, C port, a context of its own)"""
    f, cfg, cr = M.config(request.param)
    c, handle = c_config(cfg), ctypes.c_void_p()
    _lib.check(_lib.lib().pmx_ctx_create(ctypes.byref(c), 0, ctypes.byref(handle)))
    yield request.param, f, cfg, cr, Context.borrowed(cfg, 0, handle.value)
    _lib.check(_lib.lib().pmx_ctx_destroy(handle))


def _sponges(f, cfg, n, seed):
    """n sponges in mixed modes: (states, tag, index)"""
    rng = np.random.default_rng(seed)
    states = synth.random_elements(f, n * cfg.t, seed=seed).reshape(n, cfg.t, 4)
    return states, rng.integers(0, 2, n).astype(np.uint32), rng.integers(0, cfg.rate + 1, n).astype(np.uint32)


def _same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


def _cut(p, elements, length, bits):
    """mod.rs:256-286 on native elements [n][E][4] (Montgomery words): [n][length] u8, a byte per bit when `bits`"""
    rinv, n = pow(1 << 256, -1, p), elements.shape[0]
    raw = np.ascontiguousarray(elements).tobytes()
    canon = b"".join((int.from_bytes(raw[i:i + 32], "little") * rinv % p).to_bytes(32, "little") for i in range(0, len(raw), 32))
    canon = np.frombuffer(canon, dtype=np.uint8).reshape(n, -1, 32)
    per = np.unpackbits(canon, axis=-1, bitorder="little")[:, :, :p.bit_length() - 1] if bits else canon[:, :, :(p.bit_length() - 1) // 8]
    return np.ascontiguousarray(per.reshape(n, -1)[:, :length])


# ---- one checked call of every entry; `big` picks the shape that grows the blocks ---------------------------------------------------------
def permute(box, big):
    _, f, cfg, cr, ctx = box
    n = 300 if big else 1
    states = synth.random_elements(f, n * cfg.t, seed=11 + n).reshape(n, cfg.t, 4)
    assert np.array_equal(ctx.permute_batch(states), cr.permute_batch(states, threads=0))


def hash_rows(box, big):
    _, f, cfg, cr, ctx = box
    n, in_len, out_len = (200, 5, 2) if big else (1, 3, 1)
    msgs = synth.random_elements(f, n * in_len, seed=12 + n).reshape(n, in_len, 4)
    assert np.array_equal(ctx.hash_batch(msgs, in_len, out_len), cr.hash_batch(msgs, in_len, out_len, threads=0))


def absorb_squeeze(box, big, n=None, length=3):
    """absorb(length) + squeeze(length): packed below the limit, the resident walk above"""
    _, f, cfg, cr, ctx = box
    n = n or (400 if big else 1)
    states, tag, index = _sponges(f, cfg, n, seed=13 + n)
    elems = synth.random_elements(f, n * length, seed=14 + n).reshape(n, length, 4)
    want = cr.sponge_absorb_each(states, tag, index, elems, np.arange(n + 1) * length)
    ctx.sponge_absorb_batch(states, tag, index, elems, length)
    assert _same((states, tag, index), want)
    *want, want_out = cr.sponge_squeeze_each(states, tag, index, length)
    out = ctx.sponge_squeeze_batch(states, tag, index, length)
    assert np.array_equal(out, want_out) and _same((states, tag, index), want)


def squeeze_cut(box, big, n=None):
    _, f, cfg, cr, ctx = box
    p = f.modulus
    n = n or (400 if big else 1)
    for bits, length in ((False, 70 if big else 5), (True, 300 if big else 9)):
        states, tag, index = _sponges(f, cfg, n, seed=15 + n + bits)
        unit = p.bit_length() - 1 if bits else (p.bit_length() - 1) // 8
        *want, elems = cr.sponge_squeeze_each(states, tag, index, -(-length // unit))
        got = (ctx.sponge_squeeze_bits_batch if bits else ctx.sponge_squeeze_bytes_batch)(states, tag, index, length)
        assert np.array_equal(got.view(np.uint8), _cut(p, elems, length, bits)) and _same((states, tag, index), want)


def grind(box, big):
    """(its one block has one size: [state | result])"""
    _, f, cfg, cr, ctx = box
    p = f.modulus
    states, tag, index = _sponges(f, cfg, 1, seed=16 + big)
    want = None
    for v in range(64):
        s = cr.sponge_absorb(states[0], int(tag[0]), int(index[0]), f.from_ints([v]))
        if not _cut(p, cr.sponge_squeeze(*s, 1)[3].reshape(1, 1, 4), 3, True).any():
            want = v
            break
    assert ctx.sponge_grind(states[0], int(tag[0]), int(index[0]), 3, 0, 64) == want


def varlen(box, big, n=None):
    _, f, cfg, cr, ctx = box
    n = n or (300 if big else 1)
    lengths = np.random.default_rng(17 + n).integers(0, 8, n) if n > 1 else np.array([2])
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    elems = synth.random_elements(f, int(offsets[-1]), seed=18 + n)
    states, tag, index = _sponges(f, cfg, n, seed=19 + n)
    want = cr.sponge_absorb_each(states, tag, index, elems, offsets)
    ctx.sponge_absorb_varlen_batch(states, tag, index, elems, offsets)
    assert _same((states, tag, index), want)
    fresh = np.zeros((n, cfg.t, 4), dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    digests = cr.sponge_squeeze_each(*cr.sponge_absorb_each(*fresh, elems, offsets), 2)[3]
    assert np.array_equal(ctx.hash_varlen_batch(elems, offsets, 2), digests)


def matrix(box, big):
    """leaves and commitment in both layouts, then the opened rows verified with one of them wrong"""
    label, f, cfg, cr, ctx = box
    a = LABELS[label]
    n_rows, row_len = (600, 7) if big else (5, 3)
    rows = synth.random_elements(f, n_rows * row_len, seed=20 + n_rows).reshape(n_rows, row_len, 4)
    leaves = cr.hash_batch(rows, row_len, 1, threads=0).reshape(n_rows, 4)
    nodes = R.tree(cr, leaves, a)
    depth = R.shape(n_rows, a)[0]
    for layout, flat in ((_lib.MATRIX_ROW_MAJOR, rows), (_lib.MATRIX_COL_MAJOR, np.ascontiguousarray(rows.transpose(1, 0, 2)))):
        assert np.array_equal(ctx.matrix_leaves(flat, n_rows, row_len, layout), leaves)
        got_nodes, got_root = ctx.matrix_commit(flat, n_rows, row_len, layout, a)
        assert np.array_equal(got_nodes, nodes) and np.array_equal(got_root, nodes[-1])
    for k in (200,) if big else (1, 5):
        idx = R.path_indices(n_rows, a, k, seed=21 + k)
        opened, paths = rows[idx.astype(np.int64)].copy(), R.open_paths(nodes, n_rows, a, idx)
        want = np.ones(k, dtype=np.uint8)
        opened[k // 2, row_len - 1, 0] ^= 1
        want[k // 2] = 0
        assert np.array_equal(ctx.matrix_verify_rows(opened, idx, paths, depth, a, n_rows, nodes[-1]), want)


def merkle_build(box, big):
    label, f, cfg, cr, ctx = box
    a = LABELS[label]
    depth = 5 if big else 1
    leaves = synth.random_elements(f, a ** depth, seed=22 + depth)
    want = M.tree(cr, leaves, a)
    builders = [lambda: ctx.merkle_ary(leaves, a), lambda: ctx.merkle_ary_forest(leaves, 1, a)]
    if a == 2:
        builders += [lambda: ctx.merkle_2to1(leaves), lambda: ctx.merkle_2to1_forest(leaves, 1)]
    for build in builders:
        nodes, root = build()
        assert np.array_equal(nodes, want) and np.array_equal(np.asarray(root).reshape(4), want[-1])
    n = 777 if big else 1
    leaves, want = R.cached_tree(label, a, n)
    nodes, root = ctx.merkle_ragged(leaves, a)
    assert np.array_equal(nodes, want) and np.array_equal(root, want[-1])


def merkle_verify(box, big, ks=None):
    """the three verifier families; one path of each batch is wrong, so `ok` is not all ones"""
    label, f, cfg, cr, ctx = box
    a = LABELS[label]
    for k in ks or ((200,) if big else (1, 5)):
        n = 777 if big else 11
        leaves, nodes = R.cached_tree(label, a, n)
        idx = R.path_indices(n, a, k, seed=23 + k)
        mine, paths = leaves[idx.astype(np.int64)].copy(), R.open_paths(nodes, n, a, idx)
        want = np.ones(k, dtype=np.uint8)
        mine[k // 2, 1] ^= 1
        want[k // 2] = 0
        assert np.array_equal(ctx.merkle_ragged_verify_paths(mine, idx, paths, R.shape(n, a)[0], a, n, nodes[-1]), want)
        depth = 4 if big else 2
        leaves, nodes = M.cached_tree(label, a, a ** depth)
        idx = M.path_indices(a ** depth, a, k, seed=24 + k)
        mine, paths = leaves[idx.astype(np.int64)].copy(), M.open_paths(nodes, a ** depth, a, idx)
        mine[k // 2, 0] ^= 1
        assert np.array_equal(ctx.merkle_ary_verify_paths(mine, idx, paths, depth, a, nodes[-1]), want)
        if a == 2:
            ok, root = np.zeros(k, dtype=np.uint8), nodes[-1].copy()
            _lib.check(_lib.lib().pmx_merkle_verify_paths(ctx._h, _ptr(mine), _ptr(idx), _ptr(paths), depth, k, _ptr(root), _ptr(ok)))
            assert np.array_equal(ok, want)


def merkle_update(box, big):
    label, f, cfg, cr, ctx = box
    a = LABELS[label]
    depth, k = (4, 40) if big else (1, 1)
    leaves, nodes = M.cached_tree(label, a, a ** depth)
    idx = np.random.default_rng(25 + k).integers(0, a ** depth, k).astype(np.uint64)
    new = synth.random_elements(f, k, seed=26 + k)
    changed = leaves.copy()
    for i, j in enumerate(idx):
        changed[int(j)] = new[i]
    want, mine = M.tree(cr, changed, a), nodes.copy()
    root = ctx.merkle_ary_update(mine, a ** depth, a, idx, new)
    assert np.array_equal(mine, want) and np.array_equal(root, want[-1])


def merkle_fixed(box, big):
    label, f, cfg, cr, ctx = box
    a = LABELS[label]
    depth, n = (8, 150) if big else (1, 1)
    e = F.defaults(cr, F.default_leaf(label), a, depth)
    assert np.array_equal(ctx.merkle_fixed_defaults(e[0], a, depth), e)
    leaves = F.leaf_row(label, n)
    levels = F.sparse_levels(cr, leaves, a, depth, e)
    nodes, root = ctx.merkle_fixed(leaves, a, depth, e)
    assert np.array_equal(nodes, F.dense_of(levels, n, a, depth)) and np.array_equal(root, F.root_of(levels, e, depth))
    frontier, root = ctx.merkle_frontier_append(a, depth, e, None, 0, leaves)
    assert np.array_equal(frontier, F.frontier_of(levels, n, a, depth)) and np.array_equal(root, F.root_of(levels, e, depth))


ENTRIES = [permute, hash_rows, absorb_squeeze, squeeze_cut, grind, varlen, matrix, merkle_build, merkle_verify, merkle_update, merkle_fixed]


@pytest.mark.parametrize("order", ["forward", "backward"])
def test_every_entry_small_grown_small_and_then_another_entry(box, order):
    entries = ENTRIES if order == "forward" else ENTRIES[::-1]
    for entry in entries:
        entry(box, False)
        entry(box, True)
        entry(box, False)
    for entry in entries:         # every block is as large as any entry made it: each entry once more, behind a different one
        entry(box, False)


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_mode_words_on_both_sides_of_their_padding(box, n):
    """(n * 4 + 15) / 16 * 16: n = 3 pads, n = 4 fills the 16 bytes, n = 5 starts the next"""
    absorb_squeeze(box, False, n=n)
    squeeze_cut(box, False, n=n)
    varlen(box, False, n=n)


def test_the_packed_limit_and_one_sponge_more(box):
    """sponge_host packs a call of st_bytes + io_bytes + 2 * words <= 64 KiB; absorb(3) + squeeze(3)"""
    _, f, cfg, cr, ctx = box

    def packed(n):
        return n * cfg.t * 32 + n * 3 * 32 + 2 * ((n * 4 + 15) // 16 * 16)
    last = max(n for n in range(1, 2048) if packed(n) <= SMALL_CALL_BYTES)
    assert packed(last) <= SMALL_CALL_BYTES < packed(last + 1)
    absorb_squeeze(box, False, n=last)
    absorb_squeeze(box, False, n=last + 1)
    absorb_squeeze(box, False, n=last)


def test_verifiers_with_a_ragged_ok_section(box):
    """k = 1 and k = 5: `ok` [k] behind the rows (pmx_matrix_verify_rows) or alone, one path of each batch wrong"""
    merkle_verify(box, False, ks=(1, 5))
    matrix(box, False)
