"""Guard-band arenas in HOST memory for the host-buffer entry points of include/poseidon_mi355x.h (tests/test_host_arena_table.py,
tests/test_gpu_host_footprint.py).  The device arenas of tests/arena.py cover the *_dev entries; this is the other half of the ABI.  The
planner, the images and the detector are arena.plan / Plan.put / get / check / locate themselves - nothing of them is restated here.

All buffers of ONE call lie in ONE host allocation, in argument order, a guard before, between and behind them, everything poisoned with
seeded random bytes before the inputs go in.  After the call every byte outside what the header says the call writes must be unchanged:
the guards, every `const` array, the ranges `written=` excludes, and the place where an optional output that was passed as NULL would
have lain (that buffer stays in the plan with role "in"; the call gets a null pointer).

The guard is a condition, not a measurement.  A stray host write is a copy of the wrong length or at the wrong offset, and a copy is never
longer than the largest section the call stages: the largest buffer of the call, or the packed [states | io | tag | index] image of a
small sponge call (at most 64 KiB).  So
    guard = max(largest buffer of the call, 64 KiB), rounded up to 4 KiB,
and a copy that starts one whole section early or runs one whole section long still ends inside a guard.  Every case asserts this on its
own plan (guard_holds).

Placement: the natural alignment of the element type and nothing more, which is what "the host-buffer entry points accept any host
pointer" has to survive at the very least.  Field-element arrays, offsets and indices (uint64_t) get align 8 - arena.plan puts them at
8 mod 16 -, mode words and `found_out` (32-bit) at 4 mod 8, uint8_t outputs (ok, squeezed bytes / bits) at an odd address.
control=True places everything at multiples of 256, the addresses every other test passes: a failure that the control placement does not
show is an alignment fault, one that both show is a size fault.

Roles, from the header and not from the implementation: "in" every `const` array; "inout" the states and mode words of the sponge
entries, `nodes` of pmx_merkle_ary_update and the elements of pmx_to_mont / pmx_from_mont; "out" everything the header says it
"receives".  frontier_out may alias frontier_in: aliased=True lays ONE inout buffer and both arguments point at it.

Arena memory: pageable (a numpy buffer over-allocated and sliced to a 256-byte aligned base) or page-locked (pmx_host_alloc of plan.size,
wrapped without a copy, freed by close())."""
import ctypes

import numpy as np

import arena

E = arena.E
MIN_GUARD = 64 * 1024        # kSmallCallBytes: the packed image of a small sponge call
PAGE = 4096


def bind(handle, name, signatures):
    """the raw prototype `name` of a ctypes.CDLL: every pointer argument a plain address, so that it can point anywhere into an arena"""
    restype, argtypes = signatures[name]
    fn = handle[name]
    fn.restype = restype
    fn.argtypes = [ctypes.c_void_p if isinstance(a, type) and issubclass(a, ctypes._Pointer) else a for a in argtypes]
    return fn


# ---- guard and plan ------------------------------------------------------------------------------------------------------------------
def guard_for(buffers) -> int:
    largest = max([MIN_GUARD] + [nbytes for _, nbytes, _, _ in buffers])
    return (largest + PAGE - 1) // PAGE * PAGE


def plan_for(buffers, control: bool = False) -> arena.Plan:
    return arena.plan(buffers, control=control, guard=guard_for(buffers))


def guard_holds(plan: arena.Plan) -> bool:
    """the condition the guard rests on, for the plan of one call"""
    largest = max([MIN_GUARD] + [r.nbytes for r in plan.regions])
    if plan.guard < largest or plan.guard % PAGE:
        return False
    end = 0
    for r in plan.regions:
        if r.offset - end < plan.guard:
            return False
        end = r.offset + r.nbytes
    return plan.size - end >= plan.guard


class HostArena:
    """the buffers of one call in one host allocation.  alloc / free: pmx_host_alloc / pmx_host_free bound with void-pointer arguments
    (page-locked memory); None: pageable numpy memory"""

    def __init__(self, buffers, seed, control=False, alloc=None, free=None):
        self.plan = plan_for(buffers, control)
        assert guard_holds(self.plan), (self.plan.guard, [r.nbytes for r in self.plan.regions])
        self._free, self._block = free, None
        size = self.plan.size
        if alloc is None:
            self._raw = np.empty(size + arena.BASE_ALIGN, dtype=np.uint8)
            skip = -self._raw.ctypes.data % arena.BASE_ALIGN
            self.image = self._raw[skip:skip + size]
        else:
            block = ctypes.c_void_p()
            assert alloc(ctypes.byref(block), size) == 0 and block.value
            self._block = block
            self.image = np.frombuffer((ctypes.c_uint8 * size).from_address(block.value), dtype=np.uint8)
        self.base = self.image.ctypes.data
        arena.assert_base_aligned(self.base)
        self.image[:] = self.plan.poisoned(seed)
        if not control:                # the residues hold for the real addresses
            for r in self.plan.regions:
                if r.align < 32:
                    assert self.ptr(r.name) % (2 * r.align) == r.align, (r.name, hex(self.ptr(r.name)))
        self.before = None

    def put(self, name, data, at=None):
        self.plan.put(self.image, name, data, at)

    def ptr(self, name, shift=0) -> int:
        return self.plan.address(self.base, name, shift)

    def snapshot(self):
        self.before = self.image.copy()
        return self

    def finish(self, written=None):
        self.plan.check(self.before, self.image, written)

    def unchanged(self):
        assert np.array_equal(self.before, self.image), "the call changed the arena"

    def get(self, name, dtype=np.uint64):
        return self.plan.get(self.image, name, dtype)

    def close(self):
        self.image = None
        if self._block is not None:
            block, self._block = self._block, None
            assert self._free(block) == 0


# ---- the buffers of every host-buffer entry point, in argument order -----------------------------------------------------------------
def _elems(name, count, role):
    return (name, count * E, 8, role)


def _u64(name, count, role="in"):
    return (name, count * 8, 8, role)


def _opt(name, count, present):
    """an optional output: passed -> "out"; passed as NULL -> it keeps its place in the plan as "in", so a write through it is seen"""
    return (name, count * E, 8, "out" if present else "in")


def _sponges(t, n):
    return [_elems("states", n * t, "inout"), ("mode_tag", n * 4, 4, "inout"), ("mode_index", n * 4, 4, "inout")]


def permute_buffers(t, n):
    return [_elems("states", n * t, "inout")]


def hash_buffers(n, in_len, out_len):
    return [_elems("in", n * in_len, "in"), _elems("out", n * out_len, "out")]


def absorb_buffers(t, n, in_len):
    return _sponges(t, n) + [_elems("in", n * in_len, "in")]


def squeeze_buffers(t, n, out_len):
    return _sponges(t, n) + [_elems("out", n * out_len, "out")]


def hash_varlen_buffers(n, total_elems, out_len):
    return [_elems("in", total_elems, "in"), _u64("offsets", n + 1), _elems("out", n * out_len, "out")]


def absorb_varlen_buffers(t, n, total_elems):
    return _sponges(t, n) + [_elems("in", total_elems, "in"), _u64("offsets", n + 1)]


def squeeze_cut_buffers(t, n, length):
    """pmx_sponge_squeeze_bytes_batch (length = num_bytes) and pmx_sponge_squeeze_bits_batch (num_bits, a byte per bit)"""
    return _sponges(t, n) + [("out", n * length, 1, "out")]


def grind_buffers(t):
    return [_elems("state", t, "in"), _u64("nonce_out", 1, "out"), ("found_out", 4, 4, "out")]


def grind_written(found):
    """*nonce_out is not written when nothing is found"""
    return {} if found else {"nonce_out": (0, 0)}


def tree_buffers(n_trees, leaves_per_tree, nodes_per_tree, nodes=True, root=True, root_name="root"):
    """pmx_merkle_2to1 / _ary / _ragged (n_trees = 1, `root`) and their forests (`roots`): the host `nodes` receives the leaves too"""
    return [_elems("leaves", n_trees * leaves_per_tree, "in"), _opt("nodes", n_trees * nodes_per_tree, nodes),
            _opt(root_name, n_trees, root)]


def paths_buffers(n_nodes, k, depth, arity):
    """pmx_merkle_paths / _ary_paths / _ragged_paths (host-only gathers)"""
    return [_elems("nodes", n_nodes, "in"), _u64("indices", k), _elems("paths_out", k * depth * (arity - 1), "out")]


def verify_paths_buffers(k, depth, arity):
    return [_elems("leaves", k, "in"), _u64("indices", k), _elems("paths", k * depth * (arity - 1), "in"), _elems("root", 1, "in"),
            ("ok_out", k, 1, "out")]


def ary_update_buffers(n_nodes, k, root=True):
    return [_elems("nodes", n_nodes, "inout"), _u64("indices", k), _elems("new_leaves", k, "in"), _opt("root", 1, root)]


def ary_update_written(n_nodes, indices):
    """a node that is no ancestor of an updated leaf is not written at all: no leaf row below the smallest updated index is"""
    return {"nodes": (min(int(i) for i in indices) * E, n_nodes * E)}


def fixed_defaults_buffers(depth):
    return [_elems("default_leaf", 1, "in"), _elems("defaults_out", depth + 1, "out")]


def frontier_append_buffers(arity, depth, m, aliased=False, root=True):
    """frontier_in of an empty tree may be NULL: the caller then passes no pointer for it, the buffer keeps its place"""
    f = depth * (arity - 1)
    frontier = [_elems("frontier", f, "inout")] if aliased else [_elems("frontier_in", f, "in")]
    tail = [] if aliased else [_elems("frontier_out", f, "out")]
    return [_elems("defaults", depth + 1, "in")] + frontier + [_elems("new_leaves", m, "in")] + tail + [_opt("root", 1, root)]


def fixed_buffers(n_leaves, depth, n_nodes, nodes=True, root=True):
    return [_elems("leaves", n_leaves, "in"), _elems("defaults", depth + 1, "in"), _opt("nodes", n_nodes, nodes), _opt("root", 1, root)]


def fixed_paths_buffers(n_nodes, k, depth, arity):
    return [_elems("nodes", n_nodes, "in"), _elems("defaults", depth + 1, "in"), _u64("indices", k),
            _elems("paths_out", k * depth * (arity - 1), "out")]


def update_witnesses_buffers(arity, depth, k, witness=True, roots=True, root=True):
    opening = k * depth * (arity - 1)
    return [_u64("indices", k), _elems("new_leaves", k, "in"), _elems("paths", opening, "in"), _opt("witness_out", opening, witness),
            _opt("roots_out", k, roots), _opt("root", 1, root)]


def matrix_leaves_buffers(n_rows, row_len):
    return [_elems("matrix", n_rows * row_len, "in"), _elems("leaves_out", n_rows, "out")]


def matrix_commit_buffers(n_rows, row_len, n_nodes, nodes=True, root=True):
    return [_elems("matrix", n_rows * row_len, "in"), _opt("nodes", n_nodes, nodes), _opt("root", 1, root)]


def matrix_rows_buffers(n_rows, row_len, k):
    return [_elems("matrix", n_rows * row_len, "in"), _u64("indices", k), _elems("rows_out", k * row_len, "out")]


def matrix_verify_rows_buffers(row_len, k, depth, arity):
    return [_elems("rows", k * row_len, "in"), _u64("indices", k), _elems("paths", k * depth * (arity - 1), "in"), _elems("root", 1, "in"),
            ("ok_out", k, 1, "out")]


def mgpu_merkle_buffers(n_leaves):
    return [_elems("leaves", n_leaves, "in"), _elems("root", 1, "out")]


def find_ark_and_mds_buffers(rate, full_rounds, partial_rounds):
    t = rate + 1
    return [_elems("modulus", 1, "in"), _elems("ark_out", (full_rounds + partial_rounds) * t, "out"), _elems("mds_out", t * t, "out")]


def mont_constants_buffers():
    return [_elems("modulus", 1, "in"), _u64("inv", 1, "out"), _elems("r", 1, "out"), _elems("r2", 1, "out")]


def mont_convert_buffers(n):
    """pmx_to_mont / pmx_from_mont: in place"""
    return [_elems("modulus", 1, "in"), _elems("elems", n, "inout")]


def shape_buffers(names):
    """the size_t results of the *_shape functions and of pmx_shard_bounds"""
    return [_u64(name, 1, "out") for name in names]


def _ary_nodes(n_leaves, arity):
    nodes, w = n_leaves, n_leaves
    while w > 1:
        w = -(-w // arity)
        nodes += w
    return nodes


def _depth(n_leaves, arity):
    depth, w = 0, n_leaves
    while w > 1:
        w, depth = -(-w // arity), depth + 1
    return depth


def entry_point_buffers(t=3, arity=2, n=5):
    """{entry point: buffer list}: EVERY host-buffer entry point of the header at one small shape of width t, trees of `arity`, n units.
    The keys are what tests/test_host_arena_table.py counts against the prototypes of the header."""
    r = t - 1
    full, ragged, depth_fixed = arity ** 3, arity ** 3 + 1, 4
    n_full, n_ragged = _ary_nodes(full, arity), _ary_nodes(ragged, arity)
    d_full, d_ragged = _depth(full, arity), _depth(ragged, arity)
    n_fixed = sum(max(1, -(-n // arity ** l)) for l in range(depth_fixed + 1))
    return {
        "pmx_permute_batch": permute_buffers(t, n),
        "pmx_hash_batch": hash_buffers(n, r + 2, r + 1),
        "pmx_sponge_absorb_batch": absorb_buffers(t, n, r + 1),
        "pmx_sponge_squeeze_batch": squeeze_buffers(t, n, 2 * r + 1),
        "pmx_hash_varlen_batch": hash_varlen_buffers(n, 3 * n + 1, r + 1),
        "pmx_sponge_absorb_varlen_batch": absorb_varlen_buffers(t, n, 3 * n + 1),
        "pmx_sponge_squeeze_bytes_batch": squeeze_cut_buffers(t, n, 37),
        "pmx_sponge_squeeze_bits_batch": squeeze_cut_buffers(t, n, 301),
        "pmx_sponge_grind": grind_buffers(t),
        "pmx_merkle_2to1": tree_buffers(1, 8, 15),
        "pmx_merkle_2to1_forest": tree_buffers(3, 8, 15, root_name="roots"),
        "pmx_merkle_paths": paths_buffers(15, n, 3, 2),
        "pmx_merkle_verify_paths": verify_paths_buffers(n, 3, 2),
        "pmx_merkle_ary": tree_buffers(1, full, n_full),
        "pmx_merkle_ary_forest": tree_buffers(3, full, n_full, root_name="roots"),
        "pmx_merkle_ary_paths": paths_buffers(n_full, n, d_full, arity),
        "pmx_merkle_ary_verify_paths": verify_paths_buffers(n, d_full, arity),
        "pmx_merkle_ary_update": ary_update_buffers(n_full, n),
        "pmx_merkle_ragged": tree_buffers(1, ragged, n_ragged),
        "pmx_merkle_ragged_paths": paths_buffers(n_ragged, n, d_ragged, arity),
        "pmx_merkle_ragged_verify_paths": verify_paths_buffers(n, d_ragged, arity),
        "pmx_merkle_fixed_defaults": fixed_defaults_buffers(depth_fixed),
        "pmx_merkle_frontier_append": frontier_append_buffers(arity, depth_fixed, n),
        "pmx_merkle_frontier_append (aliased)": frontier_append_buffers(arity, depth_fixed, n, aliased=True),
        "pmx_merkle_fixed": fixed_buffers(n, depth_fixed, n_fixed),
        "pmx_merkle_fixed_paths": fixed_paths_buffers(n_fixed, n, depth_fixed, arity),
        "pmx_merkle_update_witnesses": update_witnesses_buffers(arity, depth_fixed, n),
        "pmx_matrix_leaves": matrix_leaves_buffers(n, 2 * r + 1),
        "pmx_matrix_commit": matrix_commit_buffers(n, 2 * r + 1, _ary_nodes(n, arity)),
        "pmx_matrix_rows": matrix_rows_buffers(n + 2, 2 * r + 1, n),
        "pmx_matrix_verify_rows": matrix_verify_rows_buffers(2 * r + 1, n, _depth(n + 2, arity), arity),
        "pmx_mgpu_permute_batch": permute_buffers(t, n),
        "pmx_mgpu_hash_batch": hash_buffers(n, r + 2, r + 1),
        "pmx_mgpu_merkle_2to1": mgpu_merkle_buffers(8),
        "pmx_find_poseidon_ark_and_mds": find_ark_and_mds_buffers(r, 8, 31),
        "pmx_mont_constants": mont_constants_buffers(),
        "pmx_to_mont": mont_convert_buffers(n),
        "pmx_from_mont": mont_convert_buffers(n),
        "pmx_merkle_ary_shape": shape_buffers(["depth", "n_nodes"]),
        "pmx_merkle_ragged_shape": shape_buffers(["depth", "n_nodes"]),
        "pmx_merkle_fixed_shape": shape_buffers(["n_nodes"]),
        "pmx_shard_bounds": shape_buffers(["start", "count"]),
    }


# ---- what the table does not hold, by name and with the reason -----------------------------------------------------------------------
EXCLUDED = {
    "pmx_host_alloc": "allocation: returns a pointer, touches no caller array",
    "pmx_host_free": "allocation: frees what pmx_host_alloc gave",
    "pmx_device_alloc": "allocation: returns a device pointer",
    "pmx_device_free": "allocation: frees a device pointer",
    "pmx_device_upload": "upload helper: one hipMemcpy of the caller's byte count, no staging of its own",
    "pmx_device_download": "download helper: one hipMemcpy of the caller's byte count, no staging of its own",
    "pmx_stream_synchronize": "takes a stream handle, no array",
    "pmx_ctx_create": "context lifetime: reads a config struct, returns a handle",
    "pmx_ctx_destroy": "context lifetime",
    "pmx_ctx_acquire": "context lifetime",
    "pmx_ctx_release": "context lifetime",
    "pmx_ctx_width": "takes a context handle, no array",
    "pmx_ctx_engine_info": "info struct of fixed size, filled on the host",
    "pmx_mgpu_unique_id": "device-group lifetime: the 128 bytes are written by the collective library",
    "pmx_mgpu_create": "device-group lifetime",
    "pmx_mgpu_create_rank": "device-group lifetime",
    "pmx_mgpu_destroy": "device-group lifetime",
    "pmx_mgpu_get_info": "info struct of fixed size, filled on the host",
    "pmx_mgpu_stream": "takes a group handle, no array",
    "pmx_mgpu_ctx": "takes a group handle, no array",
    "pmx_mgpu_synchronize": "takes a group handle, no array",
}
