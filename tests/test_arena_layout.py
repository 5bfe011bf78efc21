"""The guard-band detector of tests/arena.py must fail when it should: placement residues and guard widths for the buffer lists of
every device entry point, a clean stand-in call, and planted faults - each reported with the buffer or guard it hit.  No GPU: numpy
images and a stand-in "call" that writes what the real one would."""
import numpy as np
import pytest

import arena

WIDTHS = (2, 3, 9, 16)
RESIDUE = {16: (32, 16), 8: (16, 8), 4: (8, 4), 1: (2, 1)}     # align -> (modulus, residue)


def _lists():
    return [(t, name, bufs) for t in WIDTHS for name, bufs in arena.entry_point_buffers(t).items()]


def test_every_entry_point_is_listed_at_every_width():
    for t in WIDTHS:
        names = {n.split(" ")[0] for n in arena.entry_point_buffers(t)}
        always = {"pmx_permute_batch_dev", "pmx_hash_batch_dev", "pmx_sponge_absorb_batch_dev", "pmx_sponge_squeeze_batch_dev",
                  "pmx_sponge_absorb_varlen_batch_dev", "pmx_hash_varlen_batch_dev"}
        trees = {"pmx_merkle_2to1_dev", "pmx_merkle_2to1_forest_dev", "pmx_merkle_verify_paths_dev"}
        assert names == (always | trees if t > 2 else always), t     # rate 1: no 2-to-1 compression


@pytest.mark.parametrize("t,name,bufs", _lists(), ids=lambda v: str(v) if not isinstance(v, list) else "")
def test_residues_and_guards(t, name, bufs):
    p = arena.plan(bufs)
    assert [r.name for r in p.regions] == [b[0] for b in bufs]
    end = 0
    for r, (bname, nbytes, align, role) in zip(p.regions, bufs):
        assert (r.nbytes, r.align, r.role) == (nbytes, align, role)
        modulus, residue = RESIDUE[align]
        assert r.offset % modulus == residue, (bname, r.offset)          # the documented alignment and nothing above it
        assert r.offset - end >= arena.G, (bname, r.offset - end)        # guard before the first buffer / between two buffers
        end = r.offset + r.nbytes
    assert p.size - end >= arena.G                                       # guard behind the last one
    assert arena.G == 256 * 1024 and arena.span_fits(256, 16) and not arena.span_fits(256, 17) and not arena.span_fits(512, 16)
    # the residues are those of the real addresses for any 256-byte aligned base
    for r in p.regions:
        assert p.address(0x7F0000001300, r.name) % RESIDUE[r.align][0] == RESIDUE[r.align][1]
    with pytest.raises(AssertionError):
        arena.assert_base_aligned(0x7F0000001310)


@pytest.mark.parametrize("t,name,bufs", _lists(), ids=lambda v: str(v) if not isinstance(v, list) else "")
def test_control_layout_is_256_byte_aligned(t, name, bufs):
    p = arena.plan(bufs, control=True)
    end = 0
    for r in p.regions:
        assert r.offset % 256 == 0 and r.offset - end >= arena.G
        end = r.offset + r.nbytes
    assert p.size - end >= arena.G


# ---- a stand-in call: the absorb driver's buffers; "the kernel" overwrites states and mode words and a digest buffer -------------
def _call(p, image, rng, skip_out_element=None):
    """writes every out / inout buffer with `expected` content (as the oracle would give it); returns {name: expected bytes}"""
    expected = {}
    for r in p.regions:
        if r.role in ("out", "inout"):
            want = rng.integers(0, 256, r.nbytes, dtype=np.uint8)
            expected[r.name] = want
            got = want.copy()
            if skip_out_element is not None and r.name == skip_out_element[0]:
                e = skip_out_element[1]
                got[e * 32:(e + 1) * 32] = image[r.offset + e * 32:r.offset + (e + 1) * 32]     # this element is never stored
            image[r.offset:r.offset + r.nbytes] = got
    return expected


def _setup(seed=1, poison=True):
    t, n = 9, 65
    bufs = arena.squeeze_buffers(t, n, 2 * (t - 1) + 1)
    bufs.insert(3, ("d_in", n * 3 * 32, 16, "in"))      # an input next to the outputs
    p = arena.plan(bufs)
    rng = np.random.default_rng(seed)
    image = p.poisoned(seed, poison)
    for r in p.regions:
        if r.role in ("in", "inout"):
            p.put(image, r.name, rng.integers(0, 256, r.nbytes, dtype=np.uint8))
    return p, image, rng


def test_clean_call_passes():
    p, image, rng = _setup()
    before = image.copy()
    expected = _call(p, image, rng)
    p.check(before, image)
    for name, want in expected.items():
        assert np.array_equal(p.get(image, name, np.uint8), want)
    assert np.array_equal(p.get(image, "d_in", np.uint8), p.get(before, "d_in", np.uint8))


def test_torch_images_are_checked_like_numpy_ones():
    torch = pytest.importorskip("torch")
    p, image, rng = _setup()
    before = torch.from_numpy(image.copy())
    _call(p, image, rng)
    p.check(before, torch.from_numpy(image))
    image[p.offset("d_out") - 1] ^= 0x40
    with pytest.raises(AssertionError, match="guard before 'd_out'"):
        p.check(before, torch.from_numpy(image))


def _flip(image, offset):
    image[offset] ^= 0x01


@pytest.mark.parametrize("fault,report", [
    ("byte before d_out", r"guard before 'd_out': first differing offset (\d+), last \1, 1 byte\(s\) from"),
    ("byte behind d_out", r"guard behind 'd_out': first differing offset (\d+), last \1, 1 byte\(s\) from"),
    ("G - 1 into the guard behind d_out", rf"guard behind 'd_out': first differing offset (\d+), last \1, {arena.G - 1} byte\(s\) from"),
    ("byte inside d_in", r"buffer 'd_in' \(in\): first differing offset (\d+), last \1, 100 byte\(s\) from"),
    ("byte before d_mode_tag", r"guard before 'd_mode_tag'"),
    ("G - 1 in front of the first buffer", rf"guard before 'd_states': first differing offset (\d+), last \1, {arena.G - 1} byte\(s\) from"),
])
def test_planted_faults_are_reported_with_the_buffer_hit(fault, report):
    p, image, rng = _setup()
    before = image.copy()
    _call(p, image, rng)
    out, st, din = p["d_out"], p["d_states"], p["d_in"]
    where = {"byte before d_out": out.offset - 1, "byte behind d_out": out.offset + out.nbytes,
             "G - 1 into the guard behind d_out": out.offset + out.nbytes + arena.G - 2,     # (the last byte of the arena)
             "byte inside d_in": din.offset + 100, "byte before d_mode_tag": p.offset("d_mode_tag") - 1,
             "G - 1 in front of the first buffer": st.offset - (arena.G - 1)}[fault]
    _flip(image, where)
    with pytest.raises(AssertionError, match=report) as e:
        p.check(before, image)
    assert f"arena offsets {where} .. {where}" in str(e.value)


def test_two_faults_are_both_named_with_first_and_last_offsets():
    p, image, rng = _setup()
    before = image.copy()
    _call(p, image, rng)
    a, b = p.offset("d_states") - 32, p.offset("d_states") - 1          # one state's worth of bytes in front of the states
    image[a:b + 1] ^= 0xFF
    _flip(image, p.offset("d_in") + 7)
    with pytest.raises(AssertionError) as e:
        p.check(before, image)
    msg = str(e.value)
    assert f"guard before 'd_states': first differing offset {a}, last {b}, 1 byte(s)" in msg
    assert "buffer 'd_in' (in)" in msg and "33 byte(s) changed" in msg


@pytest.mark.parametrize("n_leaves,row", [(64, 0), (64, 63), (2, 1)])
def test_a_byte_in_the_leaves_rows_of_a_node_array_is_reported(n_leaves, row):
    p = arena.plan(arena.merkle_buffers(3, n_leaves))
    image = p.poisoned(5)
    before = image.copy()
    nodes = p["d_nodes"]
    image[nodes.offset + n_leaves * 32:nodes.offset + nodes.nbytes] ^= 0xA5        # the levels: written
    p.check(before, image, written=arena.merkle_written(n_leaves))
    _flip(image, nodes.offset + row * 32 + 5)
    with pytest.raises(AssertionError, match=r"buffer 'd_nodes' \(out\)"):
        p.check(before, image, written=arena.merkle_written(n_leaves))
    p.check(before, image)       # (without the narrowing the whole node array counts as written: the narrowing carries this case)


def test_forest_narrowing_and_a_forest_of_single_leaves():
    assert arena.forest_written(3, 16) == {"d_nodes": (48 * 32, 93 * 32)}
    p = arena.plan(arena.forest_buffers(3, 5, 1))                        # five trees of one leaf: nothing is written
    image = p.poisoned(6)
    before = image.copy()
    p.check(before, image, written=arena.forest_written(5, 1))
    _flip(image, p.offset("d_nodes") + 4 * 32)
    with pytest.raises(AssertionError, match="buffer 'd_nodes'"):
        p.check(before, image, written=arena.forest_written(5, 1))


def test_scratch_may_change_and_is_not_compared():
    p = arena.plan(arena.verify_paths_buffers(3, 6, 65))
    image = p.poisoned(7)
    before = image.copy()
    w = p["d_work"]
    image[w.offset:w.offset + w.nbytes] ^= 0xFF
    image[p.offset("d_ok"):p.offset("d_ok") + 65] = 1
    p.check(before, image)
    _flip(image, w.offset + w.nbytes)
    with pytest.raises(AssertionError, match="guard behind 'd_work'"):
        p.check(before, image)
    for name in ("d_leaves", "d_indices", "d_paths", "d_root"):
        bad = image.copy()
        _flip(bad, p.offset(name))
        with pytest.raises(AssertionError, match=f"buffer '{name}'"):
            p.check(before, bad)


@pytest.mark.parametrize("poison", [True, False], ids=["poisoned", "zero-filled"])
def test_an_unwritten_out_element_fails_the_value_comparison_because_of_the_poison(poison):
    """The kernel forgets element 7 of d_out, whose expected value happens to be zero (what a fresh torch.zeros buffer holds).  On the
    poisoned arena the value comparison sees it; on a zero-filled one it cannot - the fill is what carries this case."""
    p, image, rng = _setup(seed=3, poison=poison)
    before = image.copy()
    expected = _call(p, image, rng, skip_out_element=("d_out", 7))
    expected["d_out"][7 * 32:8 * 32] = 0
    p.check(before, image)                                # nothing outside the buffers changed: only the values can tell
    equal = np.array_equal(p.get(image, "d_out", np.uint8), expected["d_out"])
    assert equal == (not poison)
