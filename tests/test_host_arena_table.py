"""The buffer table of the host-buffer entry points (tests/host_arena.py), without a GPU:
- completeness, counted out of the header: every prototype of include/poseidon_mi355x.h with a pointer parameter is in the table, is a
  *_dev entry (the device arenas of tests/arena.py cover those) or is excluded by name with a reason;
- placement residues, guard widths and the guard condition for every list, natural and control placement;
- the entries that take no context and touch no device - the path gathers, pmx_matrix_rows, the Montgomery helpers, the parameter search,
  the *_shape functions and pmx_shard_bounds - RUN in host arenas here: outputs against the Python oracles, every other byte of the arena
  unchanged, natural and control placement, two poison seeds;
- the detector on planted faults: plain numpy writes into the "after" image of a plan from the table, each reported against the buffer
  or guard it hit.  No library is modified and nothing runs on a GPU to show that tests/test_gpu_host_footprint.py can fail: this is that
  evidence."""
import ctypes
import os
import re

import numpy as np
import pytest

from sponge_amd import _lib
from oracle import poseidon_oracle as O

import arena
import host_arena as H
import merkle_ary_oracle as MA
import merkle_fixed_oracle as MF
import merkle_ragged_oracle as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "poseidon_mi355x.h")
RESIDUE = {8: (16, 8), 4: (8, 4), 1: (2, 1)}     # align -> (modulus, residue)
E = H.E
ROW, COL = _lib.MATRIX_ROW_MAJOR, _lib.MATRIX_COL_MAJOR


# ---- completeness ----------------------------------------------------------------------------------------------------------------------
def prototypes(text):
    """{name: parameter text} of every function prototype of the header"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    found = re.findall(r"\b(?:int|void \*|pmx_ctx \*|const char \*)\s*(pmx_\w+)\s*\(([^;{}()]*)\)\s*;", text)
    return dict(found)


def with_pointer_parameter(protos):
    return {name for name, params in protos.items() if "*" in params or "[" in params}


def classify(names, table):
    """(in the table, *_dev, excluded, in none of the three, in more than one)"""
    table = {key.split(" ")[0] for key in table}
    dev = {n for n in names if n.endswith("_dev")}
    excluded = set(H.EXCLUDED)
    sets = (table, dev, excluded)
    none = {n for n in names if not any(n in s for s in sets)}
    many = {n for n in names if sum(n in s for s in sets) > 1}
    return table, dev, excluded, none, many


def test_every_prototype_with_a_pointer_parameter_is_covered_or_excluded_by_name():
    protos = prototypes(open(HEADER).read())
    assert len(protos) > 90 and "pmx_permute_batch" in protos and "pmx_mgpu_ctx" in protos and "pmx_last_error" in protos
    assert set(protos) == set(_lib.SIGNATURES)                       # the parse found what the binding declares, and nothing else
    names = with_pointer_parameter(protos)
    assert {"pmx_abi_version", "pmx_last_error", "pmx_device_count", "pmx_ctx_cache_clear"} == set(protos) - names
    table, dev, excluded, none, many = classify(names, H.entry_point_buffers())
    assert not none, f"in the header, but neither in tests/host_arena.py nor a *_dev entry nor excluded by name: {sorted(none)}"
    assert not many, sorted(many)
    assert table <= names and excluded <= names, sorted((table | excluded) - names)          # no stale name either
    assert all(len(reason) > 10 for reason in H.EXCLUDED.values())
    assert len(table) == 41 and len(excluded) == 21 and len(dev) == len(names) - 62


def test_a_prototype_missing_from_the_table_fails_the_count():
    """what commenting one table entry out does, and what a new prototype in the header does"""
    protos = prototypes(open(HEADER).read())
    names = with_pointer_parameter(protos)
    fewer = {k: v for k, v in H.entry_point_buffers().items() if k != "pmx_merkle_update_witnesses"}
    assert classify(names, fewer)[3] == {"pmx_merkle_update_witnesses"}
    more = prototypes(open(HEADER).read() + "\nint pmx_merkle_new_entry(pmx_ctx *ctx, const uint64_t *leaves,\n   size_t n, uint64_t out[PMX_LIMBS]);\n")
    assert classify(with_pointer_parameter(more), H.entry_point_buffers())[3] == {"pmx_merkle_new_entry"}
    assert "pmx_x" not in with_pointer_parameter(prototypes("int pmx_x(size_t n, int world);"))


# ---- placement -------------------------------------------------------------------------------------------------------------------------
def _lists():
    return [(t, a, name, bufs) for t, a in ((3, 2), (9, 4), (9, 8)) for name, bufs in H.entry_point_buffers(t, a).items()]


@pytest.mark.parametrize("t,a,name,bufs", _lists(), ids=lambda v: str(v) if not isinstance(v, list) else "")
def test_residues_guards_and_the_guard_condition(t, a, name, bufs):
    for control in (False, True):
        p = H.plan_for(bufs, control=control)
        assert [r.name for r in p.regions] == [b[0] for b in bufs] and H.guard_holds(p)
        assert p.guard >= H.MIN_GUARD and p.guard % H.PAGE == 0 and p.guard >= max(b[1] for b in bufs)
        end = 0
        for r in p.regions:
            assert r.align in RESIDUE and r.role in ("in", "out", "inout")
            if control:
                assert r.offset % 256 == 0
            else:
                assert r.offset % RESIDUE[r.align][0] == RESIDUE[r.align][1], (r.name, r.offset)
            assert r.offset - end >= p.guard
            end = r.offset + r.nbytes
        assert p.size - end >= p.guard
    # a plan whose guard is narrower than its largest buffer does not pass for one that holds
    big = [("a", 3 * H.MIN_GUARD, 8, "out"), ("b", 32, 8, "in")]
    assert H.guard_for(big) == 3 * H.MIN_GUARD and not H.guard_holds(arena.plan(big, guard=H.MIN_GUARD))
    assert not H.guard_holds(arena.plan(bufs, guard=H.guard_for(bufs) + 8))          # not a multiple of the page


def test_natural_types_get_their_natural_alignment():
    lists = H.entry_point_buffers()
    align = {name: {b[0]: b[2] for b in bufs} for name, bufs in lists.items()}
    assert align["pmx_sponge_absorb_batch"] == {"states": 8, "mode_tag": 4, "mode_index": 4, "in": 8}
    assert align["pmx_sponge_squeeze_bits_batch"]["out"] == 1 and align["pmx_merkle_verify_paths"]["ok_out"] == 1
    assert align["pmx_sponge_grind"] == {"state": 8, "nonce_out": 8, "found_out": 4}
    roles = {name: {b[0]: b[3] for b in bufs} for name, bufs in lists.items()}
    assert roles["pmx_merkle_ary_update"]["nodes"] == "inout" and roles["pmx_merkle_2to1"]["leaves"] == "in"
    assert roles["pmx_merkle_frontier_append (aliased)"]["frontier"] == "inout"
    assert (roles["pmx_merkle_frontier_append"]["frontier_in"], roles["pmx_merkle_frontier_append"]["frontier_out"]) == ("in", "out")
    assert {b[3] for b in H.update_witnesses_buffers(2, 4, 5, witness=False, roots=False, root=False)} == {"in"}


# ---- the pure-host entries, run in host arenas -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raw():
    handle = ctypes.CDLL(_lib.library_path())
    return lambda name: H.bind(handle, name, _lib.SIGNATURES)


def run_in_arenas(fn, buffers, inputs, expected, args, status=_lib.PMX_OK):
    """one call per placement and poison seed: the status, every expected buffer byte for byte, every other byte of the arena unchanged
    (status != PMX_OK: the whole arena)"""
    for control in (False, True):
        for seed in (1, 2):
            a = H.HostArena(buffers, seed, control=control)
            for name, data in inputs.items():
                a.put(name, data)
            a.snapshot()
            assert fn(*args(lambda name: ctypes.c_void_p(a.ptr(name)))) == status, (control, seed, _lib.lib().pmx_last_error())
            if status != _lib.PMX_OK:
                a.unchanged()
                continue
            for name, want in expected.items():
                assert a.get(name, np.uint8).tobytes() == np.ascontiguousarray(want).tobytes(), (name, control, seed)
            a.finish()
            assert H.guard_holds(a.plan)


def _indices(n, k, seed):
    idx = np.random.default_rng(seed).integers(0, n, k).astype(np.uint64)
    idx[0] = n - 1
    if k > 1:
        idx[1] = 0
    return idx


@pytest.mark.parametrize("k", [1, 5, 65])
def test_the_path_gathers_write_the_paths_and_nothing_else(raw, k):
    # pmx_merkle_paths: the 2-to-1 array of 64 leaves
    leaves, nodes = MA.cached_tree("t3", 2, 64)
    idx = _indices(64, k, 100 + k)
    run_in_arenas(raw("pmx_merkle_paths"), H.paths_buffers(127, k, 6, 2), {"nodes": nodes, "indices": idx},
                  {"paths_out": MA.open_paths(nodes, 64, 2, idx)}, lambda p: (p("nodes"), 64, p("indices"), k, p("paths_out")))
    for label, a in (("t3", 2), ("t9-bn254", 4)):
        # pmx_merkle_ary_paths: a^3 leaves
        n = a ** 3
        leaves, nodes = MA.cached_tree(label, a, n)
        idx = _indices(n, k, 200 + k)
        run_in_arenas(raw("pmx_merkle_ary_paths"), H.paths_buffers(nodes.shape[0], k, 3, a), {"nodes": nodes, "indices": idx},
                      {"paths_out": MA.open_paths(nodes, n, a, idx)}, lambda p: (p("nodes"), n, a, p("indices"), k, p("paths_out")))
        # pmx_merkle_ragged_paths: 11 leaves - the last parent of the bottom level is short at either arity
        n = 11
        assert n % a and MR.short_children(n, a)
        leaves, nodes = MR.cached_tree(label, a, n)
        idx = MR.path_indices(n, a, k, 300 + k)
        depth = MR.shape(n, a)[0]
        run_in_arenas(raw("pmx_merkle_ragged_paths"), H.paths_buffers(nodes.shape[0], k, depth, a), {"nodes": nodes, "indices": idx},
                      {"paths_out": MR.open_paths(nodes, n, a, idx)}, lambda p: (p("nodes"), n, a, p("indices"), k, p("paths_out")))
        # pmx_merkle_fixed_paths: 5 leaves in a tree of depth 4 - the siblings beyond the stored widths are e[l]
        n, depth = 5, 4
        cr = MF.config(label)[2]
        e = MF.cached_defaults(label, a, depth)
        levels = MF.sparse_levels(cr, MF.leaf_row(label, n), a, depth, e)
        dense = MF.dense_of(levels, n, a, depth)
        idx = _indices(n, k, 400 + k)
        want = MF.open_paths(levels, n, a, depth, e, idx)
        assert any((want[:, l] == e[l]).all(axis=-1).any() for l in range(depth))
        run_in_arenas(raw("pmx_merkle_fixed_paths"), H.fixed_paths_buffers(dense.shape[0], k, depth, a),
                      {"nodes": dense, "defaults": e, "indices": idx}, {"paths_out": want},
                      lambda p: (p("nodes"), n, a, depth, p("defaults"), p("indices"), k, p("paths_out")))


@pytest.mark.parametrize("k", [1, 5, 65])
@pytest.mark.parametrize("layout", [ROW, COL], ids=["row", "col"])
def test_matrix_rows_writes_the_rows_and_nothing_else(raw, layout, k):
    n_rows, row_len = 7, 3
    rows = np.random.default_rng(5).integers(0, 1 << 63, (n_rows, row_len, 4)).astype(np.uint64)
    flat = np.ascontiguousarray(rows if layout == ROW else rows.transpose(1, 0, 2))
    idx = _indices(n_rows, k, 500 + k)
    run_in_arenas(raw("pmx_matrix_rows"), H.matrix_rows_buffers(n_rows, row_len, k), {"matrix": flat, "indices": idx},
                  {"rows_out": rows[idx.astype(np.int64)]}, lambda p: (p("matrix"), n_rows, row_len, layout, p("indices"), k, p("rows_out")))


def test_a_refused_gather_leaves_its_arena_unchanged(raw):
    leaves, nodes = MA.cached_tree("t3", 2, 64)
    idx = np.array([3, 64, 1], dtype=np.uint64)                      # an index that names no leaf, behind one that does
    run_in_arenas(raw("pmx_merkle_paths"), H.paths_buffers(127, 3, 6, 2), {"nodes": nodes, "indices": idx}, {},
                  lambda p: (p("nodes"), 64, p("indices"), 3, p("paths_out")), status=_lib.PMX_ERR_ARG)
    run_in_arenas(raw("pmx_merkle_ary_paths"), H.paths_buffers(127, 3, 6, 2), {"nodes": nodes, "indices": idx}, {},
                  lambda p: (p("nodes"), 64, 2, p("indices"), 3, p("paths_out")), status=_lib.PMX_ERR_ARG)
    rows = np.zeros((7, 3, 4), dtype=np.uint64)
    idx = np.array([6, 7], dtype=np.uint64)
    run_in_arenas(raw("pmx_matrix_rows"), H.matrix_rows_buffers(7, 3, 2), {"matrix": rows, "indices": idx}, {},
                  lambda p: (p("matrix"), 7, 3, COL, p("indices"), 2, p("rows_out")), status=_lib.PMX_ERR_ARG)


def _limbs(values):
    return np.array([O.to_limbs(v) for v in values], dtype=np.uint64).reshape(len(values), 4)


@pytest.mark.parametrize("p", [O.BLS12_381_FR, O.BN254_FR], ids=["bls", "bn254"])
def test_the_montgomery_helpers_write_their_results_and_nothing_else(raw, p):
    mc = O.mont_constants(p)
    modulus = _limbs([p])
    run_in_arenas(raw("pmx_mont_constants"), H.mont_constants_buffers(), {"modulus": modulus},
                  {"inv": np.array([mc["inv"]], dtype=np.uint64), "r": _limbs([mc["r"]]), "r2": _limbs([mc["r2"]])},
                  lambda q: (q("modulus"), q("inv"), q("r"), q("r2")))
    for n in (1, 5, 65):
        values = [0, 1, p - 1, p // 3, 1 << 200][:n] + [pow(7, i, p) for i in range(max(0, n - 5))]
        canon, mont = _limbs(values), _limbs([v * mc["r"] % p for v in values])
        run_in_arenas(raw("pmx_to_mont"), H.mont_convert_buffers(n), {"modulus": modulus, "elems": canon}, {"elems": mont},
                      lambda q: (q("modulus"), q("elems"), n))
        run_in_arenas(raw("pmx_from_mont"), H.mont_convert_buffers(n), {"modulus": modulus, "elems": mont}, {"elems": canon},
                      lambda q: (q("modulus"), q("elems"), n))


def test_the_parameter_search_writes_its_tables_and_nothing_else(raw):
    cr = MA.config("t3")[2]                                            # rate 2, 8 + 31 rounds over BLS12-381: the oracle's own tables
    run_in_arenas(raw("pmx_find_poseidon_ark_and_mds"), H.find_ark_and_mds_buffers(2, 8, 31), {"modulus": _limbs([O.BLS12_381_FR])},
                  {"ark_out": cr._ark, "mds_out": cr._mds}, lambda q: (q("modulus"), 255, 2, 8, 31, 0, q("ark_out"), q("mds_out")))


def test_the_shape_functions_write_their_words_and_nothing_else(raw):
    def words(*values):
        return [np.array([v], dtype=np.uint64) for v in values]
    for n, a in ((64, 2), (64, 4), (1, 8)):
        depth, nodes = MA.shape(n, a)
        run_in_arenas(raw("pmx_merkle_ary_shape"), H.shape_buffers(["depth", "n_nodes"]), {}, dict(zip(("depth", "n_nodes"), words(depth, nodes))),
                      lambda q: (n, a, q("depth"), q("n_nodes")))
    run_in_arenas(raw("pmx_merkle_ary_shape"), H.shape_buffers(["depth", "n_nodes"]), {}, {}, lambda q: (65, 2, q("depth"), q("n_nodes")),
                  status=_lib.PMX_ERR_ARG)
    for n, a in ((11, 2), (11, 4), (777, 8)):
        depth, nodes = MR.shape(n, a)
        run_in_arenas(raw("pmx_merkle_ragged_shape"), H.shape_buffers(["depth", "n_nodes"]), {},
                      dict(zip(("depth", "n_nodes"), words(depth, nodes))), lambda q: (n, a, q("depth"), q("n_nodes")))
    for n, a, depth in ((5, 2, 4), (150, 4, 8)):
        run_in_arenas(raw("pmx_merkle_fixed_shape"), H.shape_buffers(["n_nodes"]), {}, {"n_nodes": words(sum(MF.widths(n, a, depth)))[0]},
                      lambda q: (n, a, depth, q("n_nodes")))
    for n, world, rank in ((10, 4, 1), (10, 4, 3), (7, 1, 0)):
        start = rank * (n // world) + min(rank, n % world)
        count = n // world + (rank < n % world)
        run_in_arenas(raw("pmx_shard_bounds"), H.shape_buffers(["start", "count"]), {}, dict(zip(("start", "count"), words(start, count))),
                      lambda q: (n, world, rank, q("start"), q("count")))


# ---- the detector on planted faults ------------------------------------------------------------------------------------------------------
def _stand_in(p, image, rng, written=None):
    """writes every out / inout buffer (inside `written` where it is narrowed) as the real call would"""
    for lo, hi in p.writable(written):
        image[lo:hi] = rng.integers(0, 256, hi - lo, dtype=np.uint8)


def _filled(bufs, seed=3, control=False):
    p = H.plan_for(bufs, control=control)
    rng = np.random.default_rng(seed)
    image = p.poisoned(seed)
    for r in p.regions:
        if r.role in ("in", "inout"):
            p.put(image, r.name, rng.integers(0, 256, r.nbytes, dtype=np.uint8))
    return p, image, rng


@pytest.mark.parametrize("control", [False, True], ids=["natural", "control"])
def test_one_row_past_an_out_buffer_is_reported_in_the_guard_behind_it(control):
    t, n = 9, 300
    p, image, rng = _filled(H.permute_buffers(t, n), control=control)
    before = image.copy()
    _stand_in(p, image, rng)
    p.check(before, image)
    st = p["states"]
    image[st.offset + st.nbytes:st.offset + st.nbytes + t * E] ^= 0xFF                     # a download one row too long
    with pytest.raises(AssertionError, match=rf"guard behind 'states': first differing offset {st.offset + st.nbytes}, last "
                                             rf"{st.offset + st.nbytes + t * E - 1}, 1 byte\(s\) from"):
        p.check(before, image)


def test_a_download_of_the_largest_section_at_the_wrong_buffer_ends_inside_a_guard():
    """the guard condition at work: the witness slab written one whole section early still lies in the arena"""
    bufs = H.update_witnesses_buffers(2, 32, 700)
    p, image, rng = _filled(bufs)
    w = p["witness_out"]
    assert p.guard >= w.nbytes > H.MIN_GUARD and H.guard_holds(p)
    before = image.copy()
    _stand_in(p, image, rng)
    image[w.offset - w.nbytes:w.offset] ^= 0x5A
    with pytest.raises(AssertionError, match=rf"{w.nbytes} byte\(s\) changed .*arena offsets {w.offset - w.nbytes} \.\. {w.offset - 1}") as e:
        p.check(before, image)
    assert f"guard before 'witness_out': first differing offset" in str(e.value) and f"last {w.offset - 1}, 1 byte(s)" in str(e.value)
    assert "buffer '" not in str(e.value)                   # (the guard's far half is named after the buffer it is nearer to: `paths`)


def test_a_2d_copy_whose_pitch_is_one_element_too_wide_is_reported():
    """the per-level witness slab of pmx_merkle_update_witnesses comes down as one 2-D copy: k rows of (a - 1) * 32 bytes at a pitch of
    depth * (a - 1) * 32.  With the pitch one element wider row j lands j elements late: it runs into the neighbouring levels' slots -
    inside the buffer, where only the value comparison can tell - and, from the last rows on, behind the buffer, where the detector tells."""
    a, depth, k, level = 4, 5, 65, 2
    p, image, rng = _filled(H.update_witnesses_buffers(a, depth, k))
    before = image.copy()
    _stand_in(p, image, rng)
    clean = image.copy()
    p.check(before, image)
    w, width, pitch = p["witness_out"], (a - 1) * E, depth * (a - 1) * E
    end, beyond = w.offset + w.nbytes, []
    for j in range(k):
        at = w.offset + level * width + j * (pitch + E)
        image[at:at + width] ^= 0xFF
        if at + width > end:
            beyond.append(max(at, end))
    assert beyond and beyond[-1] + width <= end + p.guard                                     # the last rows leave the buffer, not the guard
    with pytest.raises(AssertionError, match=r"guard behind 'witness_out': first differing offset (\d+)") as e:
        p.check(before, image)
    assert f"guard behind 'witness_out': first differing offset {beyond[0]}," in str(e.value)
    assert not np.array_equal(p.get(image, "witness_out", np.uint8), p.get(clean, "witness_out", np.uint8))
    # the column-major matrix slab is the same copy in the other direction: a read.  A row gathered with a pitch one element too wide
    # changes no byte of the arena; only the digests - compared with the oracle byte for byte - can tell.


@pytest.mark.parametrize("entry,name", [("pmx_hash_batch", "in"), ("pmx_merkle_update_witnesses", "paths"), ("pmx_sponge_absorb_varlen_batch", "offsets"),
                                        ("pmx_merkle_frontier_append", "defaults"), ("pmx_matrix_commit", "matrix")])
def test_a_flipped_byte_in_an_in_buffer_is_reported(entry, name):
    p, image, rng = _filled(H.entry_point_buffers(9, 4)[entry])
    before = image.copy()
    _stand_in(p, image, rng)
    p.check(before, image)
    image[p.offset(name) + 9] ^= 0x10
    with pytest.raises(AssertionError, match=rf"buffer '{name}' \(in\): first differing offset {p.offset(name) + 9}, last {p.offset(name) + 9}, 9 byte"):
        p.check(before, image)


def test_a_write_into_the_leaf_rows_that_written_excludes_is_reported():
    n_nodes, idx = 127, [40, 9, 33]
    p, image, rng = _filled(H.ary_update_buffers(n_nodes, len(idx)))
    written = H.ary_update_written(n_nodes, idx)
    assert written == {"nodes": (9 * E, 127 * E)}
    before = image.copy()
    _stand_in(p, image, rng, written)
    p.check(before, image, written)
    image[p.offset("nodes") + 8 * E + 31] ^= 0x01                                          # the last byte of leaf row 8
    with pytest.raises(AssertionError, match=r"buffer 'nodes' \(inout\)"):
        p.check(before, image, written)
    p.check(before, image)                                  # (without the narrowing the whole array counts as written)
    # and the nonce of a search that found nothing
    p, image, rng = _filled(H.grind_buffers(3))
    before = image.copy()
    _stand_in(p, image, rng, H.grind_written(False))
    p.check(before, image, H.grind_written(False))
    image[p.offset("nonce_out")] ^= 0x80
    with pytest.raises(AssertionError, match=r"buffer 'nonce_out' \(out\)"):
        p.check(before, image, H.grind_written(False))
    p.check(before, image, H.grind_written(True))


@pytest.mark.parametrize("null", ["nodes", "root", "witness_out", "roots_out"])
def test_a_write_through_where_a_null_output_would_have_lain_is_reported(null):
    if null in ("nodes", "root"):
        bufs = H.tree_buffers(1, 64, 127, nodes=null != "nodes", root=null != "root")
    else:
        bufs = H.update_witnesses_buffers(2, 6, 65, witness=null != "witness_out", roots=null != "roots_out")
    p, image, rng = _filled(bufs)
    assert p[null].role == "in"
    before = image.copy()
    _stand_in(p, image, rng)
    p.check(before, image)
    r = p[null]
    image[r.offset:r.offset + r.nbytes] = rng.integers(0, 256, r.nbytes, dtype=np.uint8)     # the call wrote it after all
    with pytest.raises(AssertionError, match=rf"buffer '{null}' \(in\): first differing offset"):
        p.check(before, image)


def test_the_arena_memory_is_base_aligned_poisoned_and_placed():
    bufs = H.absorb_buffers(3, 5, 3)
    a, b = H.HostArena(bufs, 1), H.HostArena(bufs, 2)
    assert a.base % 256 == 0 and a.ptr("states") % 16 == 8 and a.ptr("mode_tag") % 8 == 4 and a.image.shape == (a.plan.size,)
    assert not np.array_equal(a.image, b.image) and np.array_equal(a.image, H.HostArena(bufs, 1).image)
    odd = H.HostArena(H.squeeze_cut_buffers(3, 5, 37), 1)
    assert odd.ptr("out") % 2 == 1
    c = H.HostArena(bufs, 1, control=True)
    assert all(c.ptr(r.name) % 256 == 0 for r in c.plan.regions)
    a.snapshot()
    a.unchanged()
    a.image[7] ^= 1
    with pytest.raises(AssertionError, match="guard before 'states'"):
        a.finish()
