"""The HOST-memory footprint of every host-buffer entry point of include/poseidon_mi355x.h (tests/host_arena.py; the device half is
tests/test_gpu_footprint.py and its Merkle siblings).

All buffers of a call are carved out of ONE host arena - pageable numpy memory, or page-locked memory from pmx_host_alloc - at the
natural alignment of their element type and nothing above it (u64 arrays at 8 mod 16, mode words at 4 mod 8, byte outputs at an odd
address), a guard as large as the call's largest buffer (64 KiB at least) around each, everything poisoned first.  The raw ctypes
prototypes are called with addresses into the arena, never the numpy-allocating wrappers.  Every case asserts five things:
  1. the call returns PMX_OK;
  2. every out / inout buffer is byte for byte what the reference computes - the C port (oracle/cref) and the oracles built on it
     (tests/merkle_*_oracle.py, tests/merkle_chain_oracle.py, tests/grind_oracle.py), never another path of the library;
  3. Plan.check(before, after, written=...): guards, `in` buffers, unwritten ranges and the place of every output passed as NULL unchanged;
  4. the same under a second poison seed: nothing outside the inputs reached a result;
  5. the guard condition of tests/host_arena.py on the case's own plan.
One placement of every case has all buffers at multiples of 256 (the control: what every other test passes).

One context per config, made by pmx_ctx_create on the test library (the hooks live there), so that no earlier test has grown the staging
blocks: t = 3 at arity 2 (the quad engine at these sizes, the window engine above 32768 units), t = 9 over BN254 at arity 4, and at arity
8 for the witness entry.

Size classes.  S: 1 and 5 units, in both memory kinds.  M: the first shape whose staged bytes pass kSmallCallBytes (64 KiB) - for the
sponge entries the packed limit and one sponge more -, and the matrix / fixed-tree / grind entries with their hooks set so that a few
hundred rows make three slabs, pieces or chunks, the last one short.  L, for the entries whose body asks HostCall::pin (permute, hash,
the matrix entries, the witness entry): a buffer of 16 MiB or more, once in a pageable arena - where the call registers the range - and
once in a page-locked one, where the copies are chunked over three streams.  WHICH path a call took is not observable through the ABI:
the shapes are chosen from the conditions in the source, and the assertions hold on any path.  The references of the L shapes are cached
per module; a page-locked L arena is freed right after its case."""
import contextlib
import ctypes
import functools
from collections import namedtuple

import numpy as np
import pytest

from sponge_amd import _lib, synth
from sponge_amd.poseidon import c_config

import host_arena as H
import grind_oracle as G
import merkle_ary_oracle as M
import merkle_chain_oracle as C
import merkle_fixed_oracle as F
import merkle_ragged_oracle as R

pytestmark = pytest.mark.gpu

ARITY = {"t3": 2, "t9-bn254": 4}
SMALL = 64 * 1024                       # kSmallCallBytes (pmx_ctx.hpp)
PIN_MIN = 16 << 20                      # ScopedPin::kMinBytes
OK, ERR_ARG = _lib.PMX_OK, _lib.PMX_ERR_ARG
ROW, COL = _lib.MATRIX_ROW_MAJOR, _lib.MATRIX_COL_MAJOR
KINDS = ("pageable", "page-locked")
SIGNATURES = dict(_lib.SIGNATURES, **_lib.TEST_HOOK_SIGNATURES)

# entry: buffers (name, nbytes, align, role); inputs / expected {buffer: array}; args(p) -> the arguments behind the context, p(name) the
# address of a buffer (None for a name in `null`); written: what the header narrows
Case = namedtuple("Case", "entry buffers inputs expected args written null", defaults=(None, ()))
Box = namedtuple("Box", "label f cfg cr arity ctx fn")


@functools.lru_cache(maxsize=None)
def _library():
    return ctypes.CDLL(_lib.TEST_LIB_PATH)


def _fn(name):
    return H.bind(_library(), name, SIGNATURES)


@pytest.fixture(scope="module", params=list(ARITY))
def box(request):
    f, cfg, cr = M.config(request.param)
    c, handle = c_config(cfg), ctypes.c_void_p()
    assert _fn("pmx_ctx_create")(ctypes.byref(c), 0, ctypes.byref(handle)) == OK
    yield Box(request.param, f, cfg, cr, ARITY[request.param], handle, _fn)
    for hook in ("pmx_test_matrix_slab_rows", "pmx_test_merkle_fixed_piece", "pmx_test_grind_chunk"):
        _fn(hook)(0)
    assert _fn("pmx_ctx_destroy")(handle) == OK


def run(b, case, kinds=KINDS, status=OK, handle=None, control=True, whole=False):
    """every placement, memory kind and poison seed of one case; the arena of a page-locked case is freed before the next one is made.
    handle: what goes in front of the arguments instead of the box's context; whole: the call must leave the whole arena unchanged"""
    fn = _fn(case.entry)
    placements = [(kind, False, seed) for kind in kinds for seed in (1, 2)] + ([("pageable", True, 3)] if control else [])
    outputs = {}
    for kind, ctl, seed in placements:
        pinned = kind == "page-locked"
        a = H.HostArena(case.buffers, seed, control=ctl, alloc=_fn("pmx_host_alloc") if pinned else None, free=_fn("pmx_host_free"))
        try:
            for name, data in case.inputs.items():
                a.put(name, data)
            a.snapshot()
            rc = fn(b.ctx if handle is None else handle, *case.args(lambda name: None if name in case.null else ctypes.c_void_p(a.ptr(name))))
            if rc == _lib.PMX_ERR_HIP:              # the device may have faulted: nothing more is started on it in this session
                pytest.exit(f"{case.entry} ({kind}, seed {seed}): PMX_ERR_HIP: {_fn('pmx_last_error')()}", returncode=3)
            assert rc == status, (case.entry, kind, ctl, seed, rc, _fn("pmx_last_error")())
            assert H.guard_holds(a.plan)
            if status != OK or whole:
                a.unchanged()
            if status != OK:
                continue
            for name, want in case.expected.items():
                got = a.get(name, np.uint8).tobytes()
                assert got == np.ascontiguousarray(want).tobytes(), (case.entry, name, kind, ctl, seed)
                assert outputs.setdefault(name, got) == got
            a.finish(case.written)
        finally:
            a.close()


def el(b, count, seed):
    return synth.random_elements(b.f, count, seed=seed)


def first_above(row_bytes):
    """the first n whose n * row_bytes pass the small-call limit"""
    n = SMALL // row_bytes + 1
    assert (n - 1) * row_bytes <= SMALL < n * row_bytes
    return n


def sponges(b, n, seed):
    rng = np.random.default_rng(seed)
    return (el(b, n * b.cfg.t, seed).reshape(n, b.cfg.t, 4), rng.integers(0, 2, n).astype(np.uint32),
            rng.integers(0, b.cfg.rate + 1, n).astype(np.uint32))


def cut(p, elements, length, bits):
    """mod.rs:256-286 on native elements [n][E][4] (Montgomery words): [n][length] u8, a byte per bit when `bits`"""
    rinv, n = pow(1 << 256, -1, p), elements.shape[0]
    raw = np.ascontiguousarray(elements).tobytes()
    canon = b"".join((int.from_bytes(raw[i:i + 32], "little") * rinv % p).to_bytes(32, "little") for i in range(0, len(raw), 32))
    canon = np.frombuffer(canon, dtype=np.uint8).reshape(n, -1, 32)
    per = np.unpackbits(canon, axis=-1, bitorder="little")[:, :, :p.bit_length() - 1] if bits else canon[:, :, :(p.bit_length() - 1) // 8]
    return np.ascontiguousarray(per.reshape(n, -1)[:, :length])


# ---- permute and hash: S, M, L ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def permute_case(label, n):
    f, cfg, cr = M.config(label)
    states = synth.random_elements(f, n * cfg.t, seed=31 + n).reshape(n, cfg.t, 4)
    return Case("pmx_permute_batch", H.permute_buffers(cfg.t, n), {"states": states}, {"states": cr.permute_batch(states, threads=0)},
                lambda p: (p("states"), n))


@functools.lru_cache(maxsize=None)
def hash_case(label, n, in_len, out_len):
    f, cfg, cr = M.config(label)
    msgs = synth.random_elements(f, n * in_len, seed=32 + n).reshape(n, in_len, 4)
    return Case("pmx_hash_batch", H.hash_buffers(n, in_len, out_len), {"in": msgs}, {"out": cr.hash_batch(msgs, in_len, out_len, threads=0)},
                lambda p: (p("in"), in_len, p("out"), out_len, n))


def test_permute_and_hash_small_and_medium(box):
    b, t, r = box, box.cfg.t, box.cfg.rate
    for n in (1, 5, first_above(t * 32)):
        run(b, permute_case(b.label, n))
    for in_len, out_len in ((r + 1, 2), (0, 1), (2, 1)):
        for n in (1, 5, first_above(min(x for x in (in_len, out_len) if x) * 32)):
            run(b, hash_case(b.label, n, in_len, out_len))


L_PERMUTE = {"t3": (175063, 87552, 87511), "t9-bn254": (131373, 65792, 65581)}


@pytest.mark.parametrize("kind", KINDS)
def test_permute_large(box, kind):
    """>= 16 MiB of states: registered for the call (pageable) or chunked where they lie (page-locked), two chunks, the last one short and
    no multiple of 256 rows"""
    n, first, last = L_PERMUTE[box.label]
    assert n * box.cfg.t * 32 >= PIN_MIN and n >> 16 == 2 and first + last == n and first % 256 == 0 and last % 256 and first == (-(-n // 2) + 255) // 256 * 256
    run(box, permute_case(box.label, n), kinds=(kind,), control=False)


@contextlib.contextmanager
def own_box(label):
    """a context for one case (the large shapes that run at one config only)"""
    f, cfg, cr = M.config(label)
    c, handle = c_config(cfg), ctypes.c_void_p()
    assert _fn("pmx_ctx_create")(ctypes.byref(c), 0, ctypes.byref(handle)) == OK
    try:
        yield Box(label, f, cfg, cr, ARITY[label], handle, _fn)
    finally:
        assert _fn("pmx_ctx_destroy")(handle) == OK


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["in-large", "both-large"])
def test_hash_large(kind, shape):
    """`in` of 16 MiB or more with `out` below it (n >> 16 = 1: one chunk, no pipeline), and both of 16 MiB or more (two chunks).  The
    wide rows are at t = 9, the long batch at t = 3, to keep the C port's leg at a few seconds."""
    if shape == "in-large":
        label, n, in_len, out_len = "t9-bn254", 65537, 8, 1
        assert n * in_len * 32 >= PIN_MIN > n * out_len * 32 and n >> 16 == 1
    else:
        label, n, in_len, out_len = "t3", 131073, 4, 4
        assert n * in_len * 32 >= PIN_MIN and n * out_len * 32 >= PIN_MIN and n >> 16 == 2
    with own_box(label) as b:
        run(b, hash_case(label, n, in_len, out_len), kinds=(kind,), control=False)


# ---- the sponge entries -----------------------------------------------------------------------------------------------------------------
def absorb_case(b, n, length, seed=41):
    states, tag, index = sponges(b, n, seed + n)
    elems = el(b, n * length, seed + 1 + n).reshape(n, length, 4)
    st, tg, ix = b.cr.sponge_absorb_each(states, tag, index, elems, np.arange(n + 1) * length)
    return Case("pmx_sponge_absorb_batch", H.absorb_buffers(b.cfg.t, n, length), {"states": states, "mode_tag": tag, "mode_index": index, "in": elems},
                {"states": st, "mode_tag": tg, "mode_index": ix}, lambda p: (p("states"), p("mode_tag"), p("mode_index"), p("in"), length, n))


def squeeze_case(b, n, length, seed=43):
    states, tag, index = sponges(b, n, seed + n)
    st, tg, ix, out = b.cr.sponge_squeeze_each(states, tag, index, length)
    return Case("pmx_sponge_squeeze_batch", H.squeeze_buffers(b.cfg.t, n, length), {"states": states, "mode_tag": tag, "mode_index": index},
                {"states": st, "mode_tag": tg, "mode_index": ix, "out": out}, lambda p: (p("states"), p("mode_tag"), p("mode_index"), p("out"), length, n))


def squeeze_cut_case(b, n, length, bits, seed=45):
    p = b.f.modulus
    states, tag, index = sponges(b, n, seed + n + bits)
    unit = p.bit_length() - 1 if bits else (p.bit_length() - 1) // 8
    st, tg, ix, elems = b.cr.sponge_squeeze_each(states, tag, index, -(-length // unit))
    entry = "pmx_sponge_squeeze_bits_batch" if bits else "pmx_sponge_squeeze_bytes_batch"
    return Case(entry, H.squeeze_cut_buffers(b.cfg.t, n, length), {"states": states, "mode_tag": tag, "mode_index": index},
                {"states": st, "mode_tag": tg, "mode_index": ix, "out": cut(p, elems, length, bits)},
                lambda q: (q("states"), q("mode_tag"), q("mode_index"), q("out"), length, n))


def varlen_cases(b, n, seed=47):
    """(absorb, hash) over rows of 0 .. 7 elements"""
    lengths = np.random.default_rng(seed + n).integers(0, 8, n) if n > 1 else np.array([2])
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    total = int(offsets[-1])
    elems = el(b, total, seed + 1 + n)
    states, tag, index = sponges(b, n, seed + 2 + n)
    st, tg, ix = b.cr.sponge_absorb_each(states, tag, index, elems, offsets)
    absorb = Case("pmx_sponge_absorb_varlen_batch", H.absorb_varlen_buffers(b.cfg.t, n, total),
                  {"states": states, "mode_tag": tag, "mode_index": index, "in": elems, "offsets": offsets}, {"states": st, "mode_tag": tg, "mode_index": ix},
                  lambda p: (p("states"), p("mode_tag"), p("mode_index"), p("in"), p("offsets"), n))
    fresh = np.zeros((n, b.cfg.t, 4), dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    digests = b.cr.sponge_squeeze_each(*b.cr.sponge_absorb_each(*fresh, elems, offsets), 2)[3]
    hashed = Case("pmx_hash_varlen_batch", H.hash_varlen_buffers(n, total, 2), {"in": elems, "offsets": offsets}, {"out": digests},
                  lambda p: (p("in"), p("offsets"), p("out"), 2, n))
    return absorb, hashed


def packed_limit(t, length):
    """the largest n whose packed [states | io | tag | index] image is at most kSmallCallBytes (sponge_host, pmx_sponge.cpp)"""
    def packed(n):
        return n * t * 32 + n * length * 32 + 2 * ((n * 4 + 15) // 16 * 16)
    last = max(n for n in range(1, 4096) if packed(n) <= SMALL)
    assert packed(last) <= SMALL < packed(last + 1)
    return last


def test_absorb_and_squeeze_small_the_packed_limit_and_one_sponge_more(box):
    limit = packed_limit(box.cfg.t, 3)
    for n in (1, 5, limit, limit + 1):
        run(box, absorb_case(box, n, 3))
        run(box, squeeze_case(box, n, 3))
    run(box, squeeze_case(box, 5, 0))               # out_len = 0 still permutes an absorbing sponge: not an empty call


def test_squeeze_bytes_and_bits(box):
    for n in (1, 5, first_above(box.cfg.t * 32)):
        run(box, squeeze_cut_case(box, n, 5 if n < 6 else 70, False))
        run(box, squeeze_cut_case(box, n, 9 if n < 6 else 300, True))


def test_variable_length_rows(box):
    for n in (1, 5, first_above(box.cfg.t * 32)):
        for case in varlen_cases(box, n):
            run(box, case)


def grind_case(b, seed, tag, index, bits, first, count):
    hits = G.hits(b.label, seed, tag, index, first, count, bits)
    expected = {"found_out": np.array([1 if hits else 0], dtype=np.int32)}
    if hits:
        expected["nonce_out"] = np.array([hits[0]], dtype=np.uint64)
    return Case("pmx_sponge_grind", H.grind_buffers(b.cfg.t), {"state": np.array(G.sponge_state(b.label, seed))}, expected,
                lambda p: (p("state"), tag, index, bits, first, count, p("nonce_out"), p("found_out")), H.grind_written(bool(hits)))


def test_grind_found_and_not_found_in_one_chunk_and_in_several(box):
    """(its buffers have one size: a state up, a word down.)  Chunks of 20 candidates through the hook: 50 candidates are three chunks,
    the last one short; the search that finds nothing walks them all and must not write the nonce"""
    b = box
    found = grind_case(b, 1, _lib.MODE_ABSORBING, 1, 3, 1000, 50)
    nothing = grind_case(b, 1, _lib.MODE_SQUEEZING, 0, 40, 1000, 50)
    assert "nonce_out" in found.expected and "nonce_out" not in nothing.expected
    try:
        for chunk in (0, 20):
            assert b.fn("pmx_test_grind_chunk")(chunk) == OK
            run(b, found)
            run(b, nothing)
            run(b, grind_case(b, 1, _lib.MODE_ABSORBING, 1, 0, 7, 5))          # bits = 0: the first nonce, nothing launched
    finally:
        b.fn("pmx_test_grind_chunk")(0)


# ---- the tree builders and their optional outputs -----------------------------------------------------------------------------------------
def tree_case(entry, b, leaves, nodes, n_trees, extra, present, root_name="root"):
    """one builder call: `extra` the size arguments behind `leaves`, present = (nodes, root) passed or NULL"""
    per_tree = nodes.shape[0] // n_trees
    null = tuple(name for name, there in zip(("nodes", root_name), present) if not there)
    expected = {name: want for name, want, there in (("nodes", nodes, present[0]), (root_name, nodes[-n_trees:], present[1])) if there}
    return Case(entry, H.tree_buffers(n_trees, leaves.shape[0] // n_trees, per_tree, present[0], present[1], root_name), {"leaves": leaves}, expected,
                lambda p: (p("leaves"), *extra, p("nodes"), p(root_name)), None, null)


COMBOS = [(True, True), (True, False), (False, True), (False, False)]


def builder_cases(b, depth, present):
    """every builder at arity^depth leaves (and the ragged one next to it), against the C port's tree"""
    a = b.arity
    n = a ** depth
    leaves, nodes = M.cached_tree(b.label, a, n)
    cases = [tree_case("pmx_merkle_ary", b, leaves, nodes, 1, (n, a), present)]
    trees = 3
    fl = el(b, trees * n, 51 + depth)
    fn_ = M.forest(b.cr, fl, trees, a)
    cases.append(tree_case("pmx_merkle_ary_forest", b, fl, fn_, trees, (trees, n, a), present, "roots"))
    if a == 2:
        cases.append(tree_case("pmx_merkle_2to1", b, leaves, nodes, 1, (n,), present))
        cases.append(tree_case("pmx_merkle_2to1_forest", b, fl, fn_, trees, (trees, n), present, "roots"))
    m = n + 1 if n > 1 else 1
    rl, rn = R.cached_tree(b.label, a, m)
    cases.append(tree_case("pmx_merkle_ragged", b, rl, rn, 1, (m, a), present))
    return cases


def medium_depth(a):
    """the first arity^depth whose node array passes the small-call limit"""
    depth = next(d for d in range(1, 20) if M.shape(a ** d, a)[1] * 32 > SMALL)
    assert M.shape(a ** (depth - 1), a)[1] * 32 <= SMALL
    return depth


@pytest.mark.parametrize("present", COMBOS, ids=lambda c: "nodes=%d,root=%d" % c)
def test_tree_builders_with_every_combination_of_outputs(box, present):
    for depth in (0, 1, 3):                              # 1 leaf (its own root, nothing launched), one parent, a few levels
        for case in builder_cases(box, depth, present):
            run(box, case)


def test_tree_builders_medium(box):
    for case in builder_cases(box, medium_depth(box.arity), (True, True)):
        run(box, case)


def test_2to1_builders_at_the_wide_config_too(box):
    if box.arity == 2:
        return
    leaves, nodes = M.cached_tree(box.label, 2, 8)
    run(box, tree_case("pmx_merkle_2to1", box, leaves, nodes, 1, (8,), (True, True)))
    fl = el(box, 24, 52)
    run(box, tree_case("pmx_merkle_2to1_forest", box, fl, M.forest(box.cr, fl, 3, 2), 3, (3, 8), (True, True), "roots"))


# ---- verifiers ----------------------------------------------------------------------------------------------------------------------------
def verify_cases(b, k, big):
    """the three verifier families, one path of each batch wrong"""
    a = b.arity
    cases = []
    n = 777 if big else 11
    leaves, nodes = R.cached_tree(b.label, a, n)
    idx = R.path_indices(n, a, k, seed=61 + k)
    mine, paths = leaves[idx.astype(np.int64)].copy(), R.open_paths(nodes, n, a, idx)
    want = np.ones(k, dtype=np.uint8)
    mine[k // 2, 1] ^= 1
    want[k // 2] = 0
    depth = R.shape(n, a)[0]
    ins = {"leaves": mine, "indices": idx, "paths": paths, "root": nodes[-1]}
    cases.append(Case("pmx_merkle_ragged_verify_paths", H.verify_paths_buffers(k, depth, a), ins, {"ok_out": want},
                      lambda p, depth=depth, n=n: (p("leaves"), p("indices"), p("paths"), depth, a, n, k, p("root"), p("ok_out"))))
    depth = 4 if big else 2
    leaves, nodes = M.cached_tree(b.label, a, a ** depth)
    idx = M.path_indices(a ** depth, a, k, seed=62 + k)
    mine, paths = leaves[idx.astype(np.int64)].copy(), M.open_paths(nodes, a ** depth, a, idx)
    mine[k // 2, 0] ^= 1
    ins = {"leaves": mine, "indices": idx, "paths": paths, "root": nodes[-1]}
    cases.append(Case("pmx_merkle_ary_verify_paths", H.verify_paths_buffers(k, depth, a), ins, {"ok_out": want},
                      lambda p, depth=depth: (p("leaves"), p("indices"), p("paths"), depth, a, k, p("root"), p("ok_out"))))
    if a == 2:
        cases.append(Case("pmx_merkle_verify_paths", H.verify_paths_buffers(k, depth, 2), ins, {"ok_out": want},
                          lambda p, depth=depth: (p("leaves"), p("indices"), p("paths"), depth, k, p("root"), p("ok_out"))))
    return cases


def test_verifiers(box):
    for k, big in ((1, False), (5, False), (first_above(32), True)):         # M: the k leaves alone pass the limit
        for case in verify_cases(box, k, big):
            run(box, case)


# ---- leaf updates of a dense tree -----------------------------------------------------------------------------------------------------------
def update_case(b, depth, k, root=True, seed=71):
    a = b.arity
    n = a ** depth
    leaves, nodes = M.cached_tree(b.label, a, n)
    idx = np.random.default_rng(seed + k).integers(n // 2 if n > 1 else 0, n, k).astype(np.uint64)
    if k > 2:
        idx[2] = idx[0]                                     # a duplicate: the last one wins
    new = el(b, k, seed + 1 + k)
    changed = np.array(leaves)
    for i, j in enumerate(idx):
        changed[int(j)] = new[i]
    want = M.tree(b.cr, changed, a)
    expected = {"nodes": want, "root": want[-1]} if root else {"nodes": want}
    return Case("pmx_merkle_ary_update", H.ary_update_buffers(nodes.shape[0], k, root), {"nodes": nodes, "indices": idx, "new_leaves": new}, expected,
                lambda p: (p("nodes"), n, a, p("indices"), p("new_leaves"), k, p("root")), H.ary_update_written(nodes.shape[0], idx),
                () if root else ("root",))


def test_ary_update_with_and_without_a_root(box):
    for root in (True, False):
        run(box, update_case(box, 1, 1, root))
        run(box, update_case(box, 3, 5, root))
    run(box, update_case(box, medium_depth(box.arity), 40))


# ---- trees of a fixed depth -----------------------------------------------------------------------------------------------------------------
def fixed_cases(b, depth, n, present=(True, True)):
    a = b.arity
    e = F.defaults(b.cr, F.default_leaf(b.label), a, depth)
    leaves = F.leaf_row(b.label, n)
    levels = F.sparse_levels(b.cr, leaves, a, depth, e)
    dense, root = F.dense_of(levels, n, a, depth), F.root_of(levels, e, depth)
    null = tuple(name for name, there in zip(("nodes", "root"), present) if not there)
    expected = {name: want for name, want, there in (("nodes", dense, present[0]), ("root", root, present[1])) if there}
    fixed = Case("pmx_merkle_fixed", H.fixed_buffers(n, depth, dense.shape[0], *present), {"leaves": leaves, "defaults": e}, expected,
                 lambda p: (p("leaves"), n, a, depth, p("defaults"), p("nodes"), p("root")), None, null)
    defaults = Case("pmx_merkle_fixed_defaults", H.fixed_defaults_buffers(depth), {"default_leaf": e[0]}, {"defaults_out": e},
                    lambda p: (p("default_leaf"), a, depth, p("defaults_out")))
    return fixed, defaults


def append_case(b, depth, have, m, aliased, root):
    """m leaves behind `have`: from the empty tree (frontier_in NULL unless aliased) or from the oracle's frontier"""
    a = b.arity
    e = F.defaults(b.cr, F.default_leaf(b.label), a, depth)
    leaves = F.leaf_row(b.label, have + m)
    old = F.frontier_of(F.sparse_levels(b.cr, leaves[:have], a, depth, e), have, a, depth)
    levels = F.sparse_levels(b.cr, leaves, a, depth, e)
    frontier = "frontier" if aliased else "frontier_out"
    expected = {frontier: F.frontier_of(levels, have + m, a, depth)}
    if root:
        expected["root"] = F.root_of(levels, e, depth)
    null = (() if root else ("root",)) + (("frontier_in",) if have == 0 and not aliased else ())
    return Case("pmx_merkle_frontier_append", H.frontier_append_buffers(a, depth, m, aliased, root),
                {"defaults": e, "frontier" if aliased else "frontier_in": old, "new_leaves": leaves[have:]}, expected,
                lambda p: (a, depth, p("defaults"), p("frontier" if aliased else "frontier_in"), have, p("new_leaves"), m, p(frontier), p("root")),
                None, null)


@pytest.mark.parametrize("present", COMBOS, ids=lambda c: "nodes=%d,root=%d" % c)
def test_fixed_trees_with_every_combination_of_outputs(box, present):
    for depth, n in ((1, 1), (4, 5)):
        fixed, defaults = fixed_cases(box, depth, n, present)
        run(box, fixed)
        run(box, defaults)


def test_frontier_append_aliased_and_apart_with_and_without_a_root(box):
    for aliased in (False, True):
        for root in (True, False):
            run(box, append_case(box, 4, 0, 1, aliased, root))
            run(box, append_case(box, 4, 3, 5, aliased, root))
    run(box, append_case(box, 4, 5, 0, False, True))          # m = 0 is legal: the frontier again and the current root


def test_fixed_trees_medium_and_in_three_pieces(box):
    """M: the leaves pass the small-call limit.  Then 300 leaves in pieces of 128 through the hook: three pieces, the last one of 44"""
    b, depth = box, 12 if box.arity == 2 else 6
    n = first_above(32)
    assert n <= b.arity ** depth
    for case in fixed_cases(b, depth, n):
        run(b, case)
    run(b, append_case(b, depth, 3, n, False, True))
    try:
        assert b.fn("pmx_test_merkle_fixed_piece")(128) == OK
        run(b, fixed_cases(b, depth, 300)[0])
        run(b, append_case(b, depth, 7, 300, True, True))
    finally:
        b.fn("pmx_test_merkle_fixed_piece")(0)


# ---- sequential updates with witnesses ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def witness_reference(label, a, depth, k):
    """(indices, new leaves, openings, witnesses, roots): the overlay model over openings of random elements - the header defines the
    outputs by the model whatever the openings are.  Indices repeat and share ancestors."""
    f, cfg, cr = M.config(label)
    rng = np.random.default_rng(81 + k + depth)
    cap = a ** depth
    idx = np.array([int(rng.integers(0, min(cap, 4 * a))) if j % 2 else int(rng.integers(0, 1 << 62)) % cap for j in range(k)], dtype=np.uint64)
    new = synth.random_elements(f, k, seed=82 + k)
    paths = synth.random_elements(f, k * depth * (a - 1), seed=83 + k).reshape(k, depth, a - 1, 4)
    witness, roots = C.model_batched(cr, a, depth, idx, new, paths)
    return idx, new, paths, witness, roots


def witness_case(label, a, depth, k, present=(True, True, True)):
    idx, new, paths, witness, roots = witness_reference(label, a, depth, k)
    names = ("witness_out", "roots_out", "root")
    null = tuple(name for name, there in zip(names, present) if not there)
    expected = {name: want for name, want, there in zip(names, (witness, roots, roots[-1]), present) if there}
    return Case("pmx_merkle_update_witnesses", H.update_witnesses_buffers(a, depth, k, *present), {"indices": idx, "new_leaves": new, "paths": paths},
                expected, lambda p: (a, depth, p("indices"), p("new_leaves"), p("paths"), k, p("witness_out"), p("roots_out"), p("root")), None, null)


def witness_arities(b):
    return (2,) if b.label == "t3" else (4, 8)


@pytest.mark.parametrize("present", [(w, r, t) for w in (True, False) for r in (True, False) for t in (True, False)],
                         ids=lambda c: "witness=%d,roots=%d,root=%d" % c)
def test_update_witnesses_with_all_eight_combinations_of_outputs(box, present):
    for a in witness_arities(box):
        for k in (1, 5):
            run(box, witness_case(box.label, a, 6, k, present))


def test_update_witnesses_medium(box):
    """the per-level slab [k][a - 1] passes the small-call limit; it goes up and comes down as one 2-D copy per level"""
    for a in witness_arities(box):
        run(box, witness_case(box.label, a, 3, first_above((a - 1) * 32)))


@pytest.mark.parametrize("kind", KINDS)
def test_update_witnesses_large(kind):
    """depth 32, arity 2, t = 3, k = 16 385: the openings just pass 16 MiB - registered for the call, or page-locked already"""
    a, depth, k = 2, 32, 16385
    assert (k - 1) * depth * 32 == PIN_MIN
    with own_box("t3") as b:
        run(b, witness_case("t3", a, depth, k), kinds=(kind,), control=False)


# ---- matrix commitments ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrix_reference(label, a, n_rows, row_len):
    """(rows [n_rows][row_len][4], the ragged tree over their digests)"""
    f, cfg, cr = M.config(label)
    rows = synth.random_elements(f, n_rows * row_len, seed=91 + n_rows).reshape(n_rows, row_len, 4)
    return rows, R.tree(cr, cr.hash_batch(rows, row_len, 1, threads=0).reshape(n_rows, 4), a)


def matrix_cases(b, n_rows, row_len, layout, present=(True, True)):
    rows, nodes = matrix_reference(b.label, b.arity, n_rows, row_len)
    flat = np.ascontiguousarray(rows if layout == ROW else rows.transpose(1, 0, 2))
    leaves = Case("pmx_matrix_leaves", H.matrix_leaves_buffers(n_rows, row_len), {"matrix": flat}, {"leaves_out": nodes[:n_rows]},
                  lambda p: (p("matrix"), n_rows, row_len, layout, p("leaves_out")))
    null = tuple(name for name, there in zip(("nodes", "root"), present) if not there)
    expected = {name: want for name, want, there in (("nodes", nodes, present[0]), ("root", nodes[-1], present[1])) if there}
    commit = Case("pmx_matrix_commit", H.matrix_commit_buffers(n_rows, row_len, nodes.shape[0], *present), {"matrix": flat}, expected,
                  lambda p: (p("matrix"), n_rows, row_len, layout, b.arity, p("nodes"), p("root")), None, null)
    return leaves, commit


def verify_rows_case(b, n_rows, row_len, k):
    rows, nodes = matrix_reference(b.label, b.arity, n_rows, row_len)
    idx = R.path_indices(n_rows, b.arity, k, seed=92 + k)
    opened, paths = rows[idx.astype(np.int64)].copy(), R.open_paths(nodes, n_rows, b.arity, idx)
    want = np.ones(k, dtype=np.uint8)
    opened[k // 2, row_len - 1, 0] ^= 1
    want[k // 2] = 0
    depth = R.shape(n_rows, b.arity)[0]
    return Case("pmx_matrix_verify_rows", H.matrix_verify_rows_buffers(row_len, k, depth, b.arity),
                {"rows": opened, "indices": idx, "paths": paths, "root": nodes[-1]}, {"ok_out": want},
                lambda p: (p("rows"), row_len, p("indices"), p("paths"), depth, b.arity, n_rows, k, p("root"), p("ok_out")))


@pytest.mark.parametrize("layout", [ROW, COL], ids=["row", "col"])
def test_matrix_entries_small_with_every_combination_of_outputs(box, layout):
    for present in COMBOS:
        for n_rows, row_len in ((1, 3), (5, 2 * box.cfg.rate + 1)):
            leaves, commit = matrix_cases(box, n_rows, row_len, layout, present)
            run(box, commit)
    for n_rows, row_len in ((1, 3), (5, 2 * box.cfg.rate + 1)):
        run(box, matrix_cases(box, n_rows, row_len, layout)[0])


@pytest.mark.parametrize("layout", [ROW, COL], ids=["row", "col"])
def test_matrix_entries_medium_and_in_three_slabs(box, layout):
    """M: the matrix passes the small-call limit.  Then 300 rows in slabs of 128 through the hook: three slabs, the last one of 44 rows;
    a column-major slab is one 2-D copy"""
    b, row_len = box, box.cfg.rate + 1
    for case in matrix_cases(b, first_above(row_len * 32), row_len, layout):
        run(b, case)
    try:
        assert b.fn("pmx_test_matrix_slab_rows")(128) == OK
        for case in matrix_cases(b, 300, 5, layout):
            run(b, case)
    finally:
        b.fn("pmx_test_matrix_slab_rows")(0)


def test_matrix_verify_rows(box):
    for k in (1, 5):
        run(box, verify_rows_case(box, 11, 3, k))
    row_len = box.cfg.rate + 1
    run(box, verify_rows_case(box, 300, row_len, first_above(row_len * 32)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", [ROW, COL], ids=["row", "col"])
def test_matrix_large(kind, layout):
    """a matrix of 8200 rows of 64 elements at t = 9 (16.0 MiB and a little): the row-major one through pmx_matrix_leaves, the column-major
    one through pmx_matrix_commit with both outputs (its leaves are the first rows of `nodes`).  One slab of the product's size."""
    n_rows, row_len = 8200, 64
    assert n_rows * row_len * 32 >= PIN_MIN
    with own_box("t9-bn254") as b:
        run(b, matrix_cases(b, n_rows, row_len, layout)[layout == COL], kinds=(kind,), control=False)


# ---- empty and refused calls ----------------------------------------------------------------------------------------------------------------
def test_empty_calls_return_ok_and_leave_the_arena_unchanged(box):
    b, t, a = box, box.cfg.t, box.arity
    empties = [
        Case("pmx_permute_batch", H.permute_buffers(t, 0), {}, {}, lambda p: (p("states"), 0)),
        Case("pmx_hash_batch", H.hash_buffers(0, 3, 1), {}, {}, lambda p: (p("in"), 3, p("out"), 1, 0)),
        Case("pmx_sponge_absorb_batch", H.absorb_buffers(t, 0, 3), {}, {}, lambda p: (p("states"), p("mode_tag"), p("mode_index"), p("in"), 3, 0)),
        Case("pmx_sponge_squeeze_batch", H.squeeze_buffers(t, 0, 3), {}, {}, lambda p: (p("states"), p("mode_tag"), p("mode_index"), p("out"), 3, 0)),
        Case("pmx_sponge_squeeze_bytes_batch", H.squeeze_cut_buffers(t, 0, 5), {}, {}, lambda p: (p("states"), p("mode_tag"), p("mode_index"), p("out"), 5, 0)),
        Case("pmx_sponge_squeeze_bits_batch", H.squeeze_cut_buffers(t, 0, 9), {}, {}, lambda p: (p("states"), p("mode_tag"), p("mode_index"), p("out"), 9, 0)),
        Case("pmx_hash_varlen_batch", H.hash_varlen_buffers(0, 0, 2), {"offsets": np.zeros(1, dtype=np.uint64)}, {}, lambda p: (p("in"), p("offsets"), p("out"), 2, 0)),
        Case("pmx_sponge_absorb_varlen_batch", H.absorb_varlen_buffers(t, 0, 0), {"offsets": np.zeros(1, dtype=np.uint64)}, {},
             lambda p: (p("states"), p("mode_tag"), p("mode_index"), p("in"), p("offsets"), 0)),
        Case("pmx_merkle_ary_verify_paths", H.verify_paths_buffers(0, 3, a), {"root": el(b, 1, 1)}, {},
             lambda p: (p("leaves"), p("indices"), p("paths"), 3, a, 0, p("root"), p("ok_out"))),
        Case("pmx_merkle_ragged_verify_paths", H.verify_paths_buffers(0, R.shape(11, a)[0], a), {"root": el(b, 1, 1)}, {},
             lambda p: (p("leaves"), p("indices"), p("paths"), R.shape(11, a)[0], a, 11, 0, p("root"), p("ok_out"))),
        Case("pmx_matrix_verify_rows", H.matrix_verify_rows_buffers(3, 0, R.shape(11, a)[0], a), {"root": el(b, 1, 1)}, {},
             lambda p: (p("rows"), 3, p("indices"), p("paths"), R.shape(11, a)[0], a, 11, 0, p("root"), p("ok_out"))),
        Case("pmx_merkle_update_witnesses", H.update_witnesses_buffers(a, 6, 0, True, True, False), {}, {},
             lambda p: (a, 6, p("indices"), p("new_leaves"), p("paths"), 0, p("witness_out"), p("roots_out"), None)),
    ]
    state = np.array(G.sponge_state(b.label, 1))
    empties.append(Case("pmx_sponge_grind", H.grind_buffers(t), {"state": state}, {"found_out": np.zeros(1, dtype=np.int32)},
                        lambda p: (p("state"), 0, 0, 3, 5, 0, p("nonce_out"), p("found_out")), H.grind_written(False)))
    # an absorb of no elements returns before it looks at anything (mod.rs:234-236)
    states, tag, index = sponges(b, 5, 7)
    empties.append(Case("pmx_sponge_absorb_batch", H.absorb_buffers(t, 5, 0), {"states": states, "mode_tag": tag, "mode_index": index},
                        {"states": states, "mode_tag": tag, "mode_index": index}, lambda p: (p("states"), p("mode_tag"), p("mode_index"), p("in"), 0, 5)))
    leaves, nodes = M.cached_tree(b.label, a, a ** 2)
    empties.append(Case("pmx_merkle_ary_update", H.ary_update_buffers(nodes.shape[0], 0, False), {"nodes": nodes}, {"nodes": nodes},
                        lambda p: (p("nodes"), a ** 2, a, p("indices"), p("new_leaves"), 0, None)))
    if a == 2:
        empties.append(Case("pmx_merkle_verify_paths", H.verify_paths_buffers(0, 3, 2), {"root": el(b, 1, 1)}, {},
                            lambda p: (p("leaves"), p("indices"), p("paths"), 3, 0, p("root"), p("ok_out"))))
    for case in empties:
        run(b, case, control=False, whole=case.entry != "pmx_sponge_grind")    # (the empty search writes *found_out = 0, nothing else)


def test_refused_calls_give_err_arg_and_leave_the_arena_unchanged(box):
    """one documented PMX_ERR_ARG condition per entry; the arena is compared whole"""
    b, t, a, r = box, box.cfg.t, box.arity, box.cfg.rate
    n = 5
    states, tag, index = sponges(b, n, 3)
    bad_tag = tag.copy()
    bad_tag[n - 1] = 2                                                       # neither mode, on the LAST sponge
    bad_index = index.copy()
    bad_index[n - 1] = r + 1                                                 # an index above the rate
    sp = {"states": states, "mode_tag": bad_tag, "mode_index": index}
    elems = el(b, 3 * n, 4)
    down = np.array([0, 3, 2, 5, 6, 7], dtype=np.uint64)                     # offsets that decrease
    leaves, nodes = M.cached_tree(b.label, a, a ** 3)
    rl, rn = R.cached_tree(b.label, a, 11)
    e = F.defaults(b.cr, F.default_leaf(b.label), a, 2)
    full = a ** 3
    idx = np.array([1, full, 2, 0, 3], dtype=np.uint64)                      # an index that names no leaf
    vp = {"leaves": el(b, n, 5), "indices": idx, "paths": el(b, n * 3 * (a - 1), 6), "root": nodes[-1]}
    rd = R.shape(11, a)[0]
    refused = [
        Case("pmx_sponge_absorb_batch", H.absorb_buffers(t, n, 3), dict(sp, **{"in": elems}), {},
             lambda p: (p("states"), p("mode_tag"), p("mode_index"), p("in"), 3, n)),
        Case("pmx_sponge_squeeze_batch", H.squeeze_buffers(t, n, 3), dict(sp, mode_tag=tag, mode_index=bad_index), {},
             lambda p: (p("states"), p("mode_tag"), p("mode_index"), p("out"), 3, n)),
        Case("pmx_sponge_squeeze_bytes_batch", H.squeeze_cut_buffers(t, n, 5), sp, {}, lambda p: (p("states"), p("mode_tag"), p("mode_index"), p("out"), 5, n)),
        Case("pmx_sponge_squeeze_bits_batch", H.squeeze_cut_buffers(t, n, 9), sp, {}, lambda p: (p("states"), p("mode_tag"), p("mode_index"), p("out"), 9, n)),
        Case("pmx_sponge_absorb_varlen_batch", H.absorb_varlen_buffers(t, n, 7), {"states": states, "mode_tag": tag, "mode_index": index, "in": elems[:7], "offsets": down}, {},
             lambda p: (p("states"), p("mode_tag"), p("mode_index"), p("in"), p("offsets"), n)),
        Case("pmx_hash_varlen_batch", H.hash_varlen_buffers(n, 7, 2), {"in": elems[:7], "offsets": down}, {}, lambda p: (p("in"), p("offsets"), p("out"), 2, n)),
        Case("pmx_hash_varlen_batch", H.hash_varlen_buffers(1, 2, 65536 * r + r + 1), {"in": elems[:2], "offsets": np.array([0, 2], dtype=np.uint64)}, {},
             lambda p: (p("in"), p("offsets"), p("out"), 65536 * r + r + 1, 1)),          # more than 65536 rates squeezed
        Case("pmx_sponge_grind", H.grind_buffers(t), {"state": states[0]}, {}, lambda p: (p("state"), 0, 0, b.f.modulus.bit_length(), 0, 16, p("nonce_out"), p("found_out"))),
        Case("pmx_merkle_ary", H.tree_buffers(1, full, nodes.shape[0]), {"leaves": leaves}, {}, lambda p: (p("leaves"), full, 1, p("nodes"), p("root"))),
        Case("pmx_merkle_ary", H.tree_buffers(1, full, nodes.shape[0]), {"leaves": leaves}, {}, lambda p: (p("leaves"), full - 1, a, p("nodes"), p("root"))),
        Case("pmx_merkle_ary_forest", H.tree_buffers(1, full, nodes.shape[0], root_name="roots"), {"leaves": leaves}, {},
             lambda p: (p("leaves"), 1, full, 1, p("nodes"), p("roots"))),
        Case("pmx_merkle_ragged", H.tree_buffers(1, 11, rn.shape[0]), {"leaves": rl}, {}, lambda p: (p("leaves"), 11, 1, p("nodes"), p("root"))),
        Case("pmx_merkle_ragged", H.tree_buffers(1, 11, rn.shape[0]), {"leaves": rl}, {}, lambda p: (p("leaves"), 0, a, p("nodes"), p("root"))),
        Case("pmx_merkle_ary_verify_paths", H.verify_paths_buffers(n, 3, a), vp, {}, lambda p: (p("leaves"), p("indices"), p("paths"), 3, 1, n, p("root"), p("ok_out"))),
        Case("pmx_merkle_ragged_verify_paths", H.verify_paths_buffers(n, rd + 1, a), dict(vp, paths=el(b, n * (rd + 1) * (a - 1), 6)), {},
             lambda p: (p("leaves"), p("indices"), p("paths"), rd + 1, a, 11, n, p("root"), p("ok_out"))),               # a depth that is not the tree's
        Case("pmx_merkle_ary_update", H.ary_update_buffers(nodes.shape[0], n), {"nodes": nodes, "indices": idx, "new_leaves": vp["leaves"]}, {},
             lambda p: (p("nodes"), full, a, p("indices"), p("new_leaves"), n, p("root"))),
        Case("pmx_merkle_fixed_defaults", H.fixed_defaults_buffers(2), {"default_leaf": e[0]}, {}, lambda p: (p("default_leaf"), a, 0, p("defaults_out"))),
        Case("pmx_merkle_frontier_append", H.frontier_append_buffers(a, 2, n), {"defaults": e, "new_leaves": vp["leaves"]}, {},
             lambda p: (a, 2, p("defaults"), p("frontier_in"), a * a - 2, p("new_leaves"), n, p("frontier_out"), p("root"))),               # n_leaves + m > k^D
        Case("pmx_merkle_fixed", H.fixed_buffers(a * a + 1, 2, 2 * a * a), {"leaves": el(b, a * a + 1, 7), "defaults": e}, {},
             lambda p: (p("leaves"), a * a + 1, a, 2, p("defaults"), p("nodes"), p("root"))),                                    # more leaves than k^D
        Case("pmx_merkle_update_witnesses", H.update_witnesses_buffers(a, 3, n), {"indices": idx, "new_leaves": vp["leaves"], "paths": vp["paths"]}, {},
             lambda p: (a, 3, p("indices"), p("new_leaves"), p("paths"), n, p("witness_out"), p("roots_out"), p("root"))),       # an index >= a^D
        Case("pmx_merkle_update_witnesses", H.update_witnesses_buffers(a, 3, 0), {}, {},
             lambda p: (a, 3, p("indices"), p("new_leaves"), p("paths"), 0, p("witness_out"), p("roots_out"), p("root"))),       # k = 0 with a root
        Case("pmx_matrix_leaves", H.matrix_leaves_buffers(n, 3), {"matrix": elems}, {}, lambda p: (p("matrix"), n, 3, 2, p("leaves_out"))),
        Case("pmx_matrix_commit", H.matrix_commit_buffers(n, 3, R.shape(n, a)[1]), {"matrix": elems}, {}, lambda p: (p("matrix"), n, 3, COL, 1, p("nodes"), p("root"))),
        Case("pmx_matrix_verify_rows", H.matrix_verify_rows_buffers(3, n, rd + 1, a), {"rows": elems, "indices": idx, "paths": el(b, n * (rd + 1) * (a - 1), 6), "root": nodes[-1]}, {},
             lambda p: (p("rows"), 3, p("indices"), p("paths"), rd + 1, a, 11, n, p("root"), p("ok_out"))),
    ]
    if a == 2:
        refused += [
            Case("pmx_merkle_2to1", H.tree_buffers(1, 8, 15), {"leaves": leaves}, {}, lambda p: (p("leaves"), 6, p("nodes"), p("root"))),
            Case("pmx_merkle_2to1_forest", H.tree_buffers(1, 8, 15, root_name="roots"), {"leaves": leaves}, {}, lambda p: (p("leaves"), 1, 6, p("nodes"), p("roots"))),
            Case("pmx_merkle_verify_paths", H.verify_paths_buffers(n, 3, 2), vp, {}, lambda p: (p("leaves"), p("indices"), None, 3, n, p("root"), p("ok_out"))),
        ]
    for case in refused:
        run(b, case, status=ERR_ARG, control=False)
    # the two entries whose only documented argument error is a null pointer: a null context in front of good buffers
    null_ctx = ctypes.c_void_p(0)
    run(b, Case("pmx_permute_batch", H.permute_buffers(t, n), {"states": states}, {}, lambda p: (p("states"), n)), status=ERR_ARG, handle=null_ctx, control=False)
    run(b, Case("pmx_hash_batch", H.hash_buffers(n, 3, 1), {"in": elems}, {}, lambda p: (p("in"), 3, p("out"), 1, n)), status=ERR_ARG, handle=null_ctx, control=False)


# ---- the host forms of the device-group entries, on a group of one device -------------------------------------------------------------------
def test_device_group_host_entries_on_one_device(box):
    """S and M only; several devices and the stand-in collective are other tests' business"""
    b, t = box, box.cfg.t
    c, group = c_config(b.cfg), ctypes.c_void_p()
    assert _fn("pmx_mgpu_create")(ctypes.byref(c), 1, None, ctypes.byref(group)) == OK, _fn("pmx_last_error")()
    try:
        for n in (1, 5, first_above(t * 32)):
            run(b, permute_case(b.label, n)._replace(entry="pmx_mgpu_permute_batch"), handle=group)
            run(b, hash_case(b.label, n, b.cfg.rate + 1, 2)._replace(entry="pmx_mgpu_hash_batch"), handle=group)
        # 4096 leaves: 128 KiB.  First and last: the group's contexts keep the staging block, so the small trees run on a block far
        # larger than they need
        for n in (4096, 1, 8, 4096):
            leaves, nodes = M.cached_tree(b.label, 2, n)
            run(b, Case("pmx_mgpu_merkle_2to1", H.mgpu_merkle_buffers(n), {"leaves": leaves}, {"root": nodes[-1]}, lambda p: (p("leaves"), n, p("root"))),
                handle=group)
        run(b, Case("pmx_mgpu_permute_batch", H.permute_buffers(t, 0), {}, {}, lambda p: (p("states"), 0)), handle=group, control=False, whole=True)
        run(b, Case("pmx_mgpu_hash_batch", H.hash_buffers(0, 3, 1), {}, {}, lambda p: (p("in"), 3, p("out"), 1, 0)), handle=group, control=False, whole=True)
        leaves = M.cached_tree(b.label, 2, 8)[0]
        run(b, Case("pmx_mgpu_merkle_2to1", H.mgpu_merkle_buffers(8), {"leaves": leaves}, {}, lambda p: (p("leaves"), 6, p("root"))),
            handle=group, status=ERR_ARG, control=False)
        run(b, Case("pmx_mgpu_permute_batch", H.permute_buffers(t, 5), {}, {}, lambda p: (p("states"), 5)), handle=ctypes.c_void_p(0), status=ERR_ARG, control=False)
        run(b, Case("pmx_mgpu_hash_batch", H.hash_buffers(5, 3, 1), {}, {}, lambda p: (p("in"), 3, p("out"), 1, 5)), handle=ctypes.c_void_p(0), status=ERR_ARG, control=False)
    finally:
        assert _fn("pmx_mgpu_destroy")(group) == OK
