"""Guard-band arenas for the memory footprint of a call (tests/test_arena_layout.py, tests/test_gpu_footprint.py).

All buffers of ONE call are laid into ONE byte arena, G bytes of guard before, between and behind them, the whole arena poisoned with
seeded random bytes before the inputs go in.  After the call the two arena images are compared: every byte outside the regions the
call may write must be unchanged.  A stray write therefore lands inside the arena and is reported - it never leaves the allocation.

G = 256 KiB is a condition, not a measurement.  The largest span one workgroup can store is
    256 lanes x PMX_MAX_WIDTH (16) elements x 32 bytes = 128 KiB
(no kernel of this build is launched with more than 256 threads, and a lane owns at most one state), and G is twice that: a workgroup
that starts one whole span early or runs one whole span long still ends inside a guard.  Every GPU case asserts
info.threads * t * 32 <= G / 2 on the pmx_engine_info of its call (span_fits).

Placement.  A buffer of alignment a < 32 starts at an arena offset that is a multiple of a and NOT of 2 a: 16-byte buffers (states,
messages, digests, nodes) at 16 mod 32, u64 arrays (offsets, indices) at 8 mod 16, u32 arrays (mode words) at 4 mod 8, d_ok at an odd
address - the documented alignment and nothing above it, as a caller that carves its buffers out of one allocation passes them.  The
residues hold for the real addresses when the arena base is 256-byte aligned (assert_base_aligned).  control=True places everything
at multiples of 256 (the addresses every other test passes).

Roles: "in" the call must not change it; "out" the call writes every byte (expected content from the oracle); "inout" the same, starting
from valid data; "scratch" may be written, content not checked.  check(..., written={name: (lo, hi)}) narrows an out region to the byte
range the header says is written (the node rows behind the leaves of a tree); the rest of that buffer then counts as "in".

The images are numpy uint8 arrays or torch uint8 tensors (on the device the comparison runs there, on a clone of the arena; only the
offsets of differing bytes - none, when all is well - come back)."""
from collections import namedtuple

import numpy as np

G = 256 * 1024                      # guard bytes: twice the largest span one workgroup can store (see above)
MAX_WIDTH = 16                      # PMX_MAX_WIDTH
MAX_THREADS = 256                   # no kernel of this build is launched with more
assert MAX_THREADS * MAX_WIDTH * 32 == G // 2
BASE_ALIGN = 256
ROLES = ("in", "out", "inout", "scratch")

Region = namedtuple("Region", "name offset nbytes align role")


def span_fits(threads: int, t: int) -> bool:
    """the condition G rests on, for the engine of one call"""
    return threads * t * 32 <= G // 2


def assert_base_aligned(address: int) -> None:
    assert address % BASE_ALIGN == 0, f"arena base {address:#x} is not {BASE_ALIGN}-byte aligned: the residues would not hold"


def _diff_offsets(diff) -> np.ndarray:
    """offsets of the set entries of a boolean image (numpy or torch), as a numpy array"""
    if isinstance(diff, np.ndarray):
        return np.flatnonzero(diff)
    return diff.nonzero().flatten().cpu().numpy()


class Plan:
    def __init__(self, regions, size, guard, control):
        self.regions, self.size, self.guard, self.control = regions, size, guard, control
        self._by_name = {r.name: r for r in regions}

    def __getitem__(self, name) -> Region:
        return self._by_name[name]

    def offset(self, name) -> int:
        return self._by_name[name].offset

    def address(self, base: int, name: str, shift: int = 0) -> int:
        return base + self._by_name[name].offset + shift

    # ---- images --------------------------------------------------------------------------------------------------------
    def poisoned(self, seed: int, poison: bool = True) -> np.ndarray:
        """a fresh host image: seeded random bytes everywhere (poison=False: zeros - only the detector's own test asks for that, to show
        that the poison is what catches an element left unwritten)"""
        if not poison:
            return np.zeros(self.size, dtype=np.uint8)
        return np.frombuffer(np.random.default_rng(seed).bytes(self.size), dtype=np.uint8).copy()

    def put(self, image: np.ndarray, name: str, data: np.ndarray, at: int = None) -> None:
        """the whole buffer (at None: the sizes must agree), or `data` at byte offset `at` of it (the leaves rows of a node array)"""
        r = self._by_name[name]
        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        if at is None:
            assert raw.size == r.nbytes, (name, raw.size, r.nbytes)
            at = 0
        assert 0 <= at and at + raw.size <= r.nbytes, (name, at, raw.size, r.nbytes)
        image[r.offset + at:r.offset + at + raw.size] = raw

    def get(self, image, name: str, dtype=np.uint64) -> np.ndarray:
        """the bytes of one buffer as a host array of `dtype` (torch images: only this slice is downloaded)"""
        r = self._by_name[name]
        part = image[r.offset:r.offset + r.nbytes]
        if not isinstance(part, np.ndarray):
            part = part.cpu().numpy()
        return part.copy().view(dtype)

    # ---- the check -----------------------------------------------------------------------------------------------------
    def writable(self, written=None):
        """[(lo, hi)] arena byte ranges the call may change"""
        written = written or {}
        spans = []
        for r in self.regions:
            if r.name in written:
                lo, hi = written[r.name]
                assert r.role != "in" and 0 <= lo <= hi <= r.nbytes, (r.name, lo, hi)
                spans.append((r.offset + lo, r.offset + hi))
            elif r.role != "in":
                spans.append((r.offset, r.offset + r.nbytes))
        return spans

    def locate(self, offset: int):
        """(what, distance): the buffer an arena offset lies in, or the guard and the nearest buffer, and the distance in bytes to the
        nearest buffer edge (inside a buffer: to its nearer edge, counted from 0 at the first / last byte)"""
        for r in self.regions:
            if r.offset <= offset < r.offset + r.nbytes:
                return f"buffer '{r.name}' ({r.role})", min(offset - r.offset, r.offset + r.nbytes - 1 - offset)
        best = None
        for r in self.regions:
            for edge, side in ((r.offset, "before"), (r.offset + r.nbytes, "behind")):
                d = edge - offset if side == "before" else offset - edge + 1
                if d > 0 and (best is None or d < best[0]):
                    best = (d, f"guard {side} '{r.name}'")
        return best[1], best[0]

    def check(self, before, after, written=None) -> None:
        """every byte outside the regions the call may write is identical in the two images; AssertionError naming what was hit"""
        assert before.shape == after.shape == (self.size,), (before.shape, after.shape, self.size)
        diff = before != after
        for lo, hi in self.writable(written):
            diff[lo:hi] = False
        if not bool(diff.any()):
            return
        offs = _diff_offsets(diff)
        hits = {}
        for o in offs[:4096].tolist() + [int(offs[-1])]:
            what, dist = self.locate(o)
            h = hits.setdefault(what, [o, o, dist, 0])
            h[0], h[1], h[2], h[3] = min(h[0], o), max(h[1], o), min(h[2], dist), h[3] + 1
        lines = [f"{what}: first differing offset {h[0]}, last {h[1]}, {h[2]} byte(s) from the nearest buffer edge"
                 for what, h in sorted(hits.items(), key=lambda kv: kv[1][0])]
        raise AssertionError(f"{len(offs)} byte(s) changed outside the regions the call may write (arena offsets {int(offs[0])} .. "
                             f"{int(offs[-1])}):\n  " + "\n  ".join(lines))


def plan(buffers, control: bool = False, guard: int = G) -> Plan:
    """buffers: ordered [(name, nbytes, align, role)] -> their places in one arena"""
    regions, cursor = [], 0
    for name, nbytes, align, role in buffers:
        assert role in ROLES and align in (1, 2, 4, 8, 16, 32, 64, 128, 256) and nbytes >= 0, (name, nbytes, align, role)
        step = BASE_ALIGN if control else align
        offset = (cursor + guard + step - 1) // step * step
        if not control and align < 32 and (offset // align) % 2 == 0:
            offset += align                                  # a multiple of align, not of 2 align
        regions.append(Region(name, offset, nbytes, align, role))
        cursor = offset + nbytes
    return Plan(regions, cursor + guard, guard, control)


# ---- the buffers of every device entry point (include/poseidon_mi355x.h), in argument order -----------------------------------
E = 32   # bytes per field element


def permute_buffers(t, n):
    return [("d_states", n * t * E, 16, "inout")]


def hash_buffers(t, n, in_len, out_len):
    return [("d_in", n * in_len * E, 16, "in"), ("d_out", n * out_len * E, 16, "out")]


def _sponges(t, n):
    return [("d_states", n * t * E, 16, "inout"), ("d_mode_tag", n * 4, 4, "inout"), ("d_mode_index", n * 4, 4, "inout")]


def absorb_buffers(t, n, in_len):
    return _sponges(t, n) + [("d_in", n * in_len * E, 16, "in")]


def squeeze_buffers(t, n, out_len):
    return _sponges(t, n) + [("d_out", n * out_len * E, 16, "out")]


def absorb_varlen_buffers(t, n, total_elems):
    return _sponges(t, n) + [("d_in", total_elems * E, 16, "in"), ("d_offsets", (n + 1) * 8, 8, "in")]


def hash_varlen_buffers(t, n, total_elems, out_len):
    return [("d_in", total_elems * E, 16, "in"), ("d_offsets", (n + 1) * 8, 8, "in"), ("d_out", n * out_len * E, 16, "out")]


def merkle_buffers(t, n_leaves):
    return [("d_nodes", (2 * n_leaves - 1) * E, 16, "out")]


def merkle_written(n_leaves):
    """rows [n_leaves, 2 n_leaves - 1) are written; the leaves rows count as `in`"""
    return {"d_nodes": (n_leaves * E, (2 * n_leaves - 1) * E)}


def forest_buffers(t, n_trees, leaves_per_tree):
    return [("d_nodes", n_trees * (2 * leaves_per_tree - 1) * E, 16, "out")]


def forest_written(n_trees, leaves_per_tree):
    return {"d_nodes": (n_trees * leaves_per_tree * E, n_trees * (2 * leaves_per_tree - 1) * E)}


def verify_paths_buffers(t, depth, k):
    return [("d_leaves", k * E, 16, "in"), ("d_indices", k * 8, 8, "in"), ("d_paths", k * depth * E, 16, "in"), ("d_root", E, 16, "in"),
            ("d_ok", k, 1, "out"), ("d_work", k * 12 * 8, 16, "scratch")]


def entry_point_buffers(t, n=65):
    """{entry point: buffer list} at width t (rate t - 1) for n units: what tests/test_gpu_footprint.py lays out.  The (2, 1) hash shape,
    the trees and the path verifier need a rate of at least 2."""
    r = t - 1
    lists = {
        "pmx_permute_batch_dev": permute_buffers(t, n),
        "pmx_hash_batch_dev (0, 1)": hash_buffers(t, n, 0, 1),
        "pmx_hash_batch_dev (r + 2, r + 1)": hash_buffers(t, n, r + 2, r + 1),
        "pmx_sponge_absorb_batch_dev": absorb_buffers(t, n, r + 1),
        "pmx_sponge_squeeze_batch_dev": squeeze_buffers(t, n, 2 * r + 1),
        "pmx_sponge_absorb_varlen_batch_dev": absorb_varlen_buffers(t, n, 3 * r * n + 11),
        "pmx_hash_varlen_batch_dev": hash_varlen_buffers(t, n, 3 * r * n + 11, r + 1),
    }
    if r >= 2:
        lists["pmx_hash_batch_dev (2, 1)"] = hash_buffers(t, n, 2, 1)
        lists["pmx_merkle_2to1_dev"] = merkle_buffers(t, 64)
        lists["pmx_merkle_2to1_forest_dev"] = forest_buffers(t, 3, 16)
        lists["pmx_merkle_verify_paths_dev"] = verify_paths_buffers(t, 6, n)
    return lists
