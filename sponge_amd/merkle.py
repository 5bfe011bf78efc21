"""Poseidon Merkle trees on the GPU: the natural consumer of the compression mode (SURVEY section 8(f) rank 4;
the container itself lives upstream in ark-crypto-primitives, not in arkworks-rs/sponge).

A parent is  (PoseidonSponge::new; absorb(its children); squeeze_native_field_elements(1))[0]
(reference src/poseidon/mod.rs:219-254, 321-341): two children by default (pmx_merkle_2to1), `arity` of them - at most
the rate, one permutation each - with arity > 2 (pmx_merkle_ary).  Nodes are kept as one array [n_nodes][4]: leaves,
then every level, root last.  Authentication paths are verified in batch: all paths advance one level per launch."""
from __future__ import annotations

from typing import List

import numpy as np

import ctypes

from . import _lib
from .poseidon import PoseidonConfig, matrix_rows, merkle_fixed_paths, merkle_ragged_shape


class MerkleTree:
    def __init__(self, parameters: PoseidonConfig, leaves: np.ndarray, device: int = 0, arity: int = 2):
        leaves = np.ascontiguousarray(leaves, dtype=np.uint64).reshape(-1, 4)
        m = leaves.shape[0]
        assert arity >= 2, "a parent has at least two children"
        assert m >= 1, "a tree has at least one leaf"
        # any leaf count: every level has ceil(width / arity) parents, the last one absorbs the children that exist (pmx_merkle_ragged);
        # a power of the arity is the tree it always was
        self.depth, _ = merkle_ragged_shape(m, arity)
        self.ragged = m != arity ** self.depth
        self.parameters = parameters
        self.device = device
        self.arity = arity
        self.n_leaves = m
        if m == 1:
            self.nodes, self._root = leaves.copy(), leaves[0].copy()
        elif self.ragged:
            self.nodes, self._root = parameters.context(device).merkle_ragged(leaves, arity)
        elif arity == 2:
            self.nodes, self._root = parameters.context(device).merkle_2to1(leaves)
        else:
            self.nodes, self._root = parameters.context(device).merkle_ary(leaves, arity)

    @property
    def root(self) -> np.ndarray:
        return self._root

    def level_widths(self) -> List[int]:
        """nodes per level, leaves first: n, ceil(n / arity), ..., 1"""
        widths = [self.n_leaves]
        while widths[-1] > 1:
            widths.append(-(-widths[-1] // self.arity))
        return widths

    def level_offset(self, level: int) -> int:
        """Index of the first node of `level` (0 = leaves) in `nodes`: the widths of the levels below it, n + ceil(n / arity) + ..."""
        return sum(self.level_widths()[:level])

    def path(self, leaf_index: int) -> np.ndarray:
        """Siblings of the leaf, then of each ancestor, bottom-up: [depth][4] (arity 2), [depth][arity - 1][4] otherwise.  In a tree
        whose leaf count is no power of the arity a sibling that does not exist is four zero words."""
        assert 0 <= leaf_index < self.n_leaves
        return self.paths([leaf_index])[0]

    def _path_shape(self, k: int):
        return (k, self.depth, 4) if self.arity == 2 else (k, self.depth, self.arity - 1, 4)

    def paths(self, leaf_indices) -> np.ndarray:
        """[k][depth][4] for k leaves (pmx_merkle_paths: a host-side gather over the node array); with arity > 2
        [k][depth][arity - 1][4], per level the siblings in child order without the running node (pmx_merkle_ary_paths)."""
        idx = np.ascontiguousarray(leaf_indices, dtype=np.uint64)
        out = np.zeros(self._path_shape(idx.shape[0]), dtype=np.uint64)
        nodes = np.ascontiguousarray(self.nodes, dtype=np.uint64)
        if self.ragged:
            _lib.check(_lib.lib().pmx_merkle_ragged_paths(ctypes.c_void_p(nodes.ctypes.data), self.n_leaves, self.arity,
                                                          ctypes.c_void_p(idx.ctypes.data), idx.shape[0], ctypes.c_void_p(out.ctypes.data)))
        elif self.arity == 2:
            _lib.check(_lib.lib().pmx_merkle_paths(ctypes.c_void_p(nodes.ctypes.data), self.n_leaves, ctypes.c_void_p(idx.ctypes.data),
                                                   idx.shape[0], ctypes.c_void_p(out.ctypes.data)))
        else:
            _lib.check(_lib.lib().pmx_merkle_ary_paths(ctypes.c_void_p(nodes.ctypes.data), self.n_leaves, self.arity,
                                                       ctypes.c_void_p(idx.ctypes.data), idx.shape[0], ctypes.c_void_p(out.ctypes.data)))
        return out

    def update(self, leaf_indices, leaves) -> None:
        """Replace leaves leaf_indices[i] by leaves[i] and recompute only their ancestors (pmx_merkle_ary_update, any arity): `nodes`
        and `root` change in place.  Duplicate indices are sequential updates (the last one wins); an index >= n_leaves is a PmxError
        and nothing changes."""
        if not (self.nodes.dtype == np.uint64 and self.nodes.flags["C_CONTIGUOUS"] and self.nodes.flags["WRITEABLE"]):
            self.nodes = np.array(self.nodes, dtype=np.uint64, order="C")
        if self.ragged:
            return self._update_ragged(leaf_indices, leaves)
        root = self.parameters.context(self.device).merkle_ary_update(self.nodes, self.n_leaves, self.arity, leaf_indices, leaves)
        self._root[...] = root

    def _with_device_blocks(self, arrays, run, download):
        """upload `arrays` (None: an uninitialised block of that many bytes), run(pointers), download {block number: host array}"""
        L, dev = _lib.lib(), self.device
        blocks: List[ctypes.c_void_p] = []
        try:
            for a in arrays:
                d = ctypes.c_void_p()
                _lib.check(L.pmx_device_alloc(dev, ctypes.byref(d), a if isinstance(a, int) else a.nbytes))
                blocks.append(d)
                if not isinstance(a, int):
                    _lib.check(L.pmx_device_upload(dev, d, ctypes.c_void_p(a.ctypes.data), a.nbytes, None))
            run(blocks)
            for number, out in download.items():
                _lib.check(L.pmx_device_download(dev, ctypes.c_void_p(out.ctypes.data), blocks[number], out.nbytes, None))
            _lib.check(L.pmx_stream_synchronize(dev, None))
        finally:
            for d in blocks:
                L.pmx_device_free(dev, d)

    def _update_ragged(self, leaf_indices, leaves) -> None:
        """update() of a tree whose leaf count is no power of the arity: the node array goes to the device, pmx_merkle_ragged_update_dev
        runs there and the array comes back (there is no host-array entry for this layout).  The device entry ignores an index >=
        n_leaves and leaves duplicates unordered, so both are settled here: a bad index is a PmxError, the last duplicate wins."""
        idx = np.ascontiguousarray(leaf_indices, dtype=np.uint64).reshape(-1)
        new = np.ascontiguousarray(leaves, dtype=np.uint64).reshape(-1, 4)
        assert new.shape[0] == idx.shape[0], "one new leaf per index"
        bad = idx[idx >= np.uint64(self.n_leaves)]
        if bad.size:
            raise _lib.PmxError(_lib.PMX_ERR_ARG, f"leaf index {int(bad[0])} out of range")
        if idx.size == 0:
            return
        last = {int(i): n for n, i in enumerate(idx)}                  # index -> its last update
        keep = np.array(sorted(last.values()), dtype=np.int64)
        idx, new = np.ascontiguousarray(idx[keep]), np.ascontiguousarray(new[keep])
        k, ctx = idx.shape[0], self.parameters.context(self.device)
        self._with_device_blocks(
            [self.nodes, idx, new, k * (self.arity + 1) * 32],
            lambda d: ctx.merkle_ragged_update_dev(d[0], self.n_leaves, self.arity, d[1], d[2], k, d[3], None),
            {0: self.nodes})
        self._root[...] = self.nodes[-1]

    def paths_dev(self, leaf_indices) -> np.ndarray:
        """paths() through the device-side gather (pmx_merkle_ary_paths_dev): node array and indices are uploaded, the paths
        gathered there and downloaded.  (A caller whose node array already lives on the device calls
        Context.merkle_ary_paths_dev on its own pointers; this is that call with the copies around it.)  Unlike paths(), an
        index >= n_leaves is not an error here: its path comes back all zero."""
        idx = np.ascontiguousarray(leaf_indices, dtype=np.uint64)
        out = np.zeros(self._path_shape(idx.shape[0]), dtype=np.uint64)
        if out.size == 0:
            return out
        nodes = np.ascontiguousarray(self.nodes, dtype=np.uint64)
        ctx = self.parameters.context(self.device)
        gather = ctx.merkle_ragged_paths_dev if self.ragged else ctx.merkle_ary_paths_dev
        self._with_device_blocks([nodes, idx, out.nbytes], lambda d: gather(d[0], self.n_leaves, self.arity, d[1], idx.shape[0], d[2], None), {2: out})
        return out


def _default_leaf(parameters: PoseidonConfig, default_leaf) -> np.ndarray:
    """an integer is a field element (converted to the library's form), anything else is the element's four words"""
    if isinstance(default_leaf, (int, np.integer)):
        return np.ascontiguousarray(parameters.field.from_ints([int(default_leaf)]), dtype=np.uint64).reshape(4)
    return np.ascontiguousarray(default_leaf, dtype=np.uint64).reshape(4)


class FixedMerkleTree:
    """The dense tree of a fixed depth over n >= 1 leaves, every other of the arity^depth positions a default leaf (pmx_merkle_fixed;
    MerkleTree.fixed makes it): `.nodes` holds the complete and the partial nodes of every level, leaves first and root last,
    `.defaults` [depth + 1][4] the digests of the empty subtrees, `.open(indices)` the openings [k][depth][arity - 1][4], which
    verify_paths(..., arity=arity) of a tree of arity^depth leaves accepts (at arity 2: reshape to [k][depth][4])."""

    def __init__(self, parameters: PoseidonConfig, leaves, depth: int, arity: int = 2, default_leaf=0, device: int = 0):
        leaves = np.ascontiguousarray(leaves, dtype=np.uint64).reshape(-1, 4)
        ctx = parameters.context(device)
        self.parameters, self.device, self.arity, self.depth, self.n_leaves = parameters, device, arity, depth, leaves.shape[0]
        self.defaults = ctx.merkle_fixed_defaults(_default_leaf(parameters, default_leaf), arity, depth)
        self.nodes, self._root = ctx.merkle_fixed(leaves, arity, depth, self.defaults)

    @property
    def root(self) -> np.ndarray:
        return self._root

    def open(self, indices) -> np.ndarray:
        return merkle_fixed_paths(self.nodes, self.n_leaves, self.arity, self.depth, self.defaults, indices)


MerkleTree.fixed = staticmethod(lambda parameters, leaves, depth, arity=2, default_leaf=0, device=0:
                                FixedMerkleTree(parameters, leaves, depth, arity, default_leaf, device))


class IncrementalMerkleTree:
    """An append-only tree of a fixed depth (a note-commitment tree, an identity group, a rollup's state tree): what is kept is the
    frontier - depth * (arity - 1) digests - and the leaf count; `.append(leaves)` is pmx_merkle_frontier_append, at most `depth`
    compression launches per piece whatever the number of leaves.  `.root` is the root of the tree padded with the default leaf."""

    def __init__(self, parameters: PoseidonConfig, depth: int, arity: int = 2, default_leaf=0, device: int = 0):
        self.parameters, self.device, self.arity, self.depth = parameters, device, arity, depth
        self.defaults = parameters.context(device).merkle_fixed_defaults(_default_leaf(parameters, default_leaf), arity, depth)
        self.frontier = np.zeros((depth, arity - 1, 4), dtype=np.uint64)
        self.n_leaves = 0
        self._root = self.defaults[depth].copy()

    @property
    def root(self) -> np.ndarray:
        return self._root

    def append(self, leaves) -> np.ndarray:
        """append leaves [m][4]; returns the new root"""
        leaves = np.ascontiguousarray(leaves, dtype=np.uint64).reshape(-1, 4)
        if leaves.shape[0] == 0:
            return self._root
        self.frontier, self._root = self.parameters.context(self.device).merkle_frontier_append(
            self.arity, self.depth, self.defaults, self.frontier, self.n_leaves, leaves)
        self.n_leaves += leaves.shape[0]
        return self._root


def update_witnesses(parameters: PoseidonConfig, depth: int, indices, new_leaves, paths, arity: int = 2, device: int = 0):
    """k sequential leaf updates of a tree of `arity` and fixed `depth` (a rollup's state tree) from the openings of the k indices in the
    tree BEFORE the batch, paths [k][depth][arity - 1][4] as FixedMerkleTree.open gives them (pmx_merkle_update_witnesses; `depth`
    compression launches of k rows whatever k).  Returns (witnesses, roots): witnesses[j] [depth][arity - 1][4] is the opening of
    indices[j] in the tree after updates 0 .. j - 1, roots[j] [4] the root after update j; roots[-1] is the final root.  Duplicate
    indices are sequential updates of one leaf.  The paths are not checked against an old root: that is verify_paths."""
    wit, roots, _ = parameters.context(device).merkle_update_witnesses(arity, depth, indices, new_leaves, paths)
    return wit, roots


def verify_paths(parameters: PoseidonConfig, leaves: np.ndarray, indices, paths: np.ndarray, root: np.ndarray,
                 device: int = 0, arity: int = 2, n_leaves: int = None) -> np.ndarray:
    """k authentication paths at once: leaves [k][4], indices [k], paths [k][depth][4] -> bool[k]
    (pmx_merkle_verify_paths: one upload, one device step per level, one download; an index with bits at or above
    `depth` names no leaf and verifies as False).  With arity > 2 paths are [k][depth][arity - 1][4]
    (pmx_merkle_ary_verify_paths; an index >= arity^depth verifies as False).
    n_leaves: the leaf count of a tree over any number of leaves (pmx_merkle_ragged_verify_paths; paths [k][depth][arity - 1][4], or
    [k][depth][4] at arity 2): the root does not bind it, so the verifier states it, and an index >= n_leaves verifies as False."""
    cur = np.ascontiguousarray(leaves, dtype=np.uint64).reshape(-1, 4)
    idx = np.ascontiguousarray(indices, dtype=np.uint64)
    paths = np.ascontiguousarray(paths, dtype=np.uint64)
    k = cur.shape[0]
    root = np.ascontiguousarray(root, dtype=np.uint64).reshape(4)
    ctx = parameters.context(device)
    if n_leaves is not None:
        depth, _ = merkle_ragged_shape(n_leaves, arity)
        assert paths.size == k * depth * (arity - 1) * 4, "paths are [k][depth][arity - 1][4] for the depth of (n_leaves, arity)"
        return ctx.merkle_ragged_verify_paths(cur, idx, paths, depth, arity, n_leaves, root).astype(bool)
    if arity != 2:
        depth = paths.shape[1] if paths.ndim == 4 else 0
        return ctx.merkle_ary_verify_paths(cur, idx, paths, depth, arity, root).astype(bool)
    depth = paths.shape[1] if paths.ndim == 3 else 0
    ok = np.zeros(k, dtype=np.uint8)
    _lib.check(_lib.lib().pmx_merkle_verify_paths(ctx._h, ctypes.c_void_p(cur.ctypes.data), ctypes.c_void_p(idx.ctypes.data),
                                                  ctypes.c_void_p(paths.ctypes.data) if paths.size else None, depth, k,
                                                  ctypes.c_void_p(root.ctypes.data), ctypes.c_void_p(ok.ctypes.data)))
    return ok.astype(bool)


LAYOUTS = {"row": _lib.MATRIX_ROW_MAJOR, "col": _lib.MATRIX_COL_MAJOR}


class MatrixCommitment:
    """The commitment a STARK / FRI prover makes to a trace or LDE matrix: every ROW is hashed to a digest, leaf_i = (new; absorb(row i);
    squeeze_native(1))[0], and the digests are the leaves of a tree of `arity` over any number of rows (pmx_matrix_commit: the matrix
    goes up in slabs, is hashed where it lies and the leaves never leave the device).

    matrix is the array as it lies in memory: layout "col" (one column per polynomial, the usual one) [row_len][n_rows][4], layout "row"
    [n_rows][row_len][4].  Nothing is transposed.  `.tree` is the MerkleTree over the digests (its nodes are those of the call),
    `.root` its root, `.open(indices)` the opened rows - row-major, [k][row_len][4] - with their authentication paths."""

    def __init__(self, parameters: PoseidonConfig, matrix: np.ndarray, layout: str = "col", arity: int = 2, device: int = 0):
        assert layout in LAYOUTS, "layout is 'col' or 'row'"
        matrix = np.ascontiguousarray(matrix, dtype=np.uint64)
        assert matrix.ndim == 3 and matrix.shape[2] == 4, "a matrix is [row_len][n_rows][4] ('col') or [n_rows][row_len][4] ('row')"
        self.layout = LAYOUTS[layout]
        self.row_len, self.n_rows = matrix.shape[:2] if layout == "col" else matrix.shape[1::-1]
        self.matrix, self.parameters, self.device, self.arity = matrix, parameters, device, arity
        nodes, root = parameters.context(device).matrix_commit(matrix, self.n_rows, self.row_len, self.layout, arity)
        self.tree = MerkleTree.__new__(MerkleTree)          # the tree of the digests, from the nodes this call brought back
        self.tree.parameters, self.tree.device, self.tree.arity, self.tree.n_leaves = parameters, device, arity, self.n_rows
        self.tree.depth, _ = merkle_ragged_shape(self.n_rows, arity)
        self.tree.ragged = self.n_rows != arity ** self.tree.depth
        self.tree.nodes, self.tree._root = nodes, root

    @property
    def root(self) -> np.ndarray:
        return self.tree.root

    def open(self, indices):
        """(rows [k][row_len][4], paths): the opened rows (pmx_matrix_rows) and the paths of their digests (MerkleTree.paths)"""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        return matrix_rows(self.matrix, self.n_rows, self.row_len, self.layout, idx), self.tree.paths(idx)


def verify_rows(parameters: PoseidonConfig, rows: np.ndarray, indices, paths: np.ndarray, root: np.ndarray, n_rows: int, arity: int = 2,
                device: int = 0) -> np.ndarray:
    """k opened rows [k][row_len][4] against the root of a MatrixCommitment over n_rows rows: bool[k] (pmx_matrix_verify_rows - one hash
    launch over the rows, then the climb of verify_paths).  The root does not bind n_rows, so the verifier states it; an index >= n_rows
    verifies as False."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    assert rows.ndim == 3 and rows.shape[2] == 4, "rows are [k][row_len][4]"
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    paths = np.ascontiguousarray(paths, dtype=np.uint64)
    root = np.ascontiguousarray(root, dtype=np.uint64).reshape(4)
    depth, _ = merkle_ragged_shape(n_rows, arity)
    assert paths.size == idx.shape[0] * depth * (arity - 1) * 4, "paths are [k][depth][arity - 1][4] for the depth of (n_rows, arity)"
    return parameters.context(device).matrix_verify_rows(rows, idx, paths, depth, arity, n_rows, root).astype(bool)


def matrix_view_extent(n_rows: int, row_len: int, row_stride: int, elem_stride: int) -> int:
    """the elements a strided view of a matrix on the device spans, 1 + (n_rows - 1) * row_stride + (row_len - 1) * elem_stride
    (pmx_matrix_view_extent: host only; an empty dimension, a zero stride or a byte size beyond size_t is a PmxError)"""
    extent = ctypes.c_size_t()
    _lib.check(_lib.lib().pmx_matrix_view_extent(n_rows, row_len, row_stride, elem_stride, ctypes.byref(extent)))
    return extent.value


class DeviceMatrixCommitment:
    """MatrixCommitment for a matrix that already lives on the device (include/poseidon_mi355x_resident.h): `ptr` is a raw device address
    and the matrix a strided view of it, element (i, j) at ptr + (i * row_stride + j * elem_stride) * 32 bytes - (1, ld) column-major as
    an NTT leaves it, (row_len, 1) row-major, a block of a larger matrix.  Nothing is copied or transposed, and nothing comes to the
    host: the constructor enqueues pmx_matrix_commit_dev on `stream` (None: the default stream) into a node array this object owns
    (pmx_device_alloc), `.root_ptr` is the device address of the root, `.open` and `.verify_rows_dev` enqueue on the same stream.
    No torch here: a caller that holds its memory in torch tensors passes data_ptr() and torch.cuda.current_stream().cuda_stream.
    `.close()` frees what the object allocated (the node array and what open() handed out) once the stream's work is done."""

    def __init__(self, parameters: PoseidonConfig, ptr: int, n_rows: int, row_len: int, row_stride: int, elem_stride: int, arity: int = 2,
                 stream=None, device: int = 0):
        self.parameters, self.device, self.stream = parameters, device, stream
        self.ptr, self.n_rows, self.row_len, self.row_stride, self.elem_stride, self.arity = ptr, n_rows, row_len, row_stride, elem_stride, arity
        self.extent = matrix_view_extent(n_rows, row_len, row_stride, elem_stride)
        self.depth, self.n_nodes = merkle_ragged_shape(n_rows, arity)
        self._blocks: List[ctypes.c_void_p] = []
        self.nodes_ptr = self._alloc(self.n_nodes * 32)
        try:
            self._ctx().matrix_commit_dev(ptr, n_rows, row_len, row_stride, elem_stride, arity, self.nodes_ptr, stream)
        except _lib.PmxError:
            self.close()
            raise

    def _ctx(self):
        return self.parameters.context(self.device)

    def _alloc(self, nbytes: int) -> int:
        d = ctypes.c_void_p()
        _lib.check(_lib.lib().pmx_device_alloc(self.device, ctypes.byref(d), max(nbytes, 32)))
        self._blocks.append(d)
        return d.value

    @property
    def root_ptr(self) -> int:
        """device address of the root [4]: the last row of the node array"""
        return self.nodes_ptr + (self.n_nodes - 1) * 32

    def open(self, d_indices_ptr: int, k: int, with_paths: bool = True):
        """(d_rows, d_paths): device addresses of the k opened rows [k][row_len][4] and of their paths [k][depth][arity - 1][4] (None
        without paths) for the k u64 indices at d_indices_ptr, which never leave the device (pmx_matrix_open_dev).  An index >= n_rows
        gets an all-zero row and path.  The blocks belong to this object."""
        d_rows = self._alloc(k * self.row_len * 32)
        d_paths = self._alloc(k * self.depth * (self.arity - 1) * 32) if with_paths else None
        self._ctx().matrix_open_dev(self.ptr, self.n_rows, self.row_len, self.row_stride, self.elem_stride,
                                    self.nodes_ptr if with_paths else None, self.arity, d_indices_ptr, k, d_rows, d_paths, self.stream)
        return d_rows, d_paths

    def verify_rows_dev(self, d_rows: int, d_indices_ptr: int, d_paths: int, k: int, d_ok: int, d_root: int = None, d_work: int = None) -> None:
        """d_ok[i] = 1 iff opened row i climbs its path to the root (this commitment's unless d_root is given) and its index is below
        n_rows (pmx_matrix_verify_rows_dev).  d_work: [k][(arity + 2) * 4] u64 of scratch, allocated here when not given."""
        if d_work is None:
            d_work = self._alloc(k * (self.arity + 2) * 32)
        self._ctx().matrix_verify_rows_dev(d_rows, self.row_len, d_indices_ptr, d_paths, self.depth, self.arity, self.n_rows, k,
                                           self.root_ptr if d_root is None else d_root, d_ok, d_work, self.stream)

    def close(self) -> None:
        L = _lib.lib()
        if self._blocks:
            L.pmx_stream_synchronize(self.device, self.stream)
        for d in self._blocks:
            L.pmx_device_free(self.device, d)
        self._blocks = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
