"""Trees over ANY number of leaves, their openings and path climbs from the oracle's C restatement (oracle/cref), for
tests/test_merkle_ragged_host.py, tests/test_gpu_merkle_ragged.py and tests/test_gpu_merkle_ragged_footprint.py.  Nothing here calls the
product.  Configs and labels are those of tests/merkle_ary_oracle.py.

Level l + 1 has ceil(M_l / a) nodes.  A full parent is CRef.hash_batch(children [1][a][4], a, 1); the SHORT last parent of a level is
CRef.hash_batch(children [1][r][4], r, 1) - new; absorb(the r children that exist); squeeze_native(1) (src/poseidon/mod.rs:126-135,
219-230, 324-328) - and never a row padded with zeros: that the two agree is what the product's tests check, not what they assume.
Node arrays are the leaves, then every level, root last; paths are [k][depth][a - 1][4], bottom-up, per level the siblings in child order
with the running node's own slot left out and four zero words for a sibling that does not exist."""
import functools

import numpy as np

from sponge_amd import synth

import merkle_ary_oracle as M

config = M.config
CONFIGS = M.CONFIGS


def widths(n_leaves, a):
    """nodes per level, leaves first: n, ceil(n / a), ..., 1"""
    w = [n_leaves]
    while w[-1] > 1:
        w.append(-(-w[-1] // a))
    return w


def shape(n_leaves, a):
    """(depth, n_nodes) by plain arithmetic"""
    w = widths(n_leaves, a)
    return len(w) - 1, sum(w)


def parents(cr, level, a):
    """the next level: the full rows in one batch, then the short row - if any - as an absorb of its r children"""
    level = np.ascontiguousarray(level, dtype=np.uint64).reshape(-1, 4)
    full, r = divmod(level.shape[0], a)
    out = []
    if full:
        out.append(cr.hash_batch(level[:full * a].reshape(full, a, 4), a, 1, threads=0).reshape(full, 4))
    if r:
        out.append(cr.hash_batch(level[full * a:].reshape(1, r, 4), r, 1, threads=0).reshape(1, 4))
    return np.concatenate(out)


def tree(cr, leaves, a):
    levels = [np.ascontiguousarray(leaves, dtype=np.uint64).reshape(-1, 4)]
    while levels[-1].shape[0] > 1:
        levels.append(parents(cr, levels[-1], a))
    return np.concatenate(levels)


@functools.lru_cache(maxsize=None)
def cached_tree(label, a, n_leaves, seed=0):
    """(leaves, nodes) of the tree every test of one case shares; read-only"""
    f, cfg, cr = config(label)
    leaves = synth.random_elements(f, n_leaves, seed=0xA99ED + 1000 * a + n_leaves + seed)
    nodes = tree(cr, leaves, a)
    leaves.setflags(write=False)
    nodes.setflags(write=False)
    return leaves, nodes


def open_paths(nodes, n_leaves, a, indices):
    """[k][depth][a - 1][4] by the index arithmetic of the header, one sibling at a time; an absent sibling stays zero"""
    w = widths(n_leaves, a)
    out = np.zeros((len(indices), len(w) - 1, a - 1, 4), dtype=np.uint64)
    for i, index in enumerate(int(x) for x in indices):
        assert index < n_leaves
        first, idx = 0, index
        for level in range(len(w) - 1):
            digit, base = idx % a, idx - idx % a
            for s, c in enumerate(c for c in range(a) if c != digit):
                if base + c < w[level]:
                    out[i, level, s] = nodes[first + base + c]
            first, idx = first + w[level], idx // a
    return out


def climb(cr, leaves, indices, paths, a, n_leaves):
    """hash leaves [k][4] up their paths as the TREE does: the running node's parent absorbs the children that exist at its level - the
    running node at digit (index / a^level) % a and the siblings below the level's width - so an absent sibling's words are never read.
    Indices below n_leaves.  Returns the k top nodes."""
    w = widths(n_leaves, a)
    k = paths.shape[0]
    cur = np.ascontiguousarray(leaves, dtype=np.uint64).reshape(k, 4).copy()
    for i in range(k):
        idx = int(indices[i])
        assert idx < n_leaves
        for level in range(len(w) - 1):
            digit, base = idx % a, idx - idx % a
            have = min(a, w[level] - base)
            row = np.zeros((have, 4), dtype=np.uint64)
            for c in range(have):
                row[c] = cur[i] if c == digit else paths[i, level, c if c < digit else c - 1]
            cur[i] = cr.hash_batch(row.reshape(1, have, 4), have, 1, threads=1).reshape(4)
            idx //= a
    return cur


def short_children(n_leaves, a):
    """[(level, child index in its level)]: every child of the short parent of every level that has one, and the last child of the full
    parent next to it"""
    out = []
    for level, width in enumerate(widths(n_leaves, a)[:-1]):
        r = width % a
        if r:
            out += [(level, width - r + c) for c in range(r)]
            if width > r:
                out.append((level, width - r - 1))
    return out


def path_indices(n_leaves, a, k, seed):
    """k leaf indices that include n - 1, 0, a leaf under every child of the short parent of every level and under a child of the full
    parent next to it (the first leaf of node c of level l is c * a^l), then random ones"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_leaves, k).astype(np.uint64)
    must = [n_leaves - 1, 0] + [c * a ** level for level, c in short_children(n_leaves, a)]
    for slot, value in enumerate(must[:k]):
        assert value < n_leaves
        idx[slot] = value
    return idx
