"""Trees, openings and path climbs of any arity from the oracle's C restatement (oracle/cref), for tests/test_merkle_ary_host.py,
tests/test_gpu_merkle_ary.py and tests/test_gpu_merkle_ary_footprint.py.  Nothing here calls the product.

A parent is CRef.hash_batch(children [1][a][4], a, 1): new; absorb(a children); squeeze_native(1) (src/poseidon/mod.rs:126-135, 219-230,
324-328).  Node arrays are the leaves, then every level, root last; a forest is level-major (level l of every tree, tree after tree);
paths are [k][depth][a - 1][4], bottom-up, per level the siblings in child order with the running node's own slot left out."""
import functools

import numpy as np

import sponge_amd as S
from sponge_amd import synth
from oracle import cref
from oracle import poseidon_oracle as O

FIELD = {"bls": (S.BLS12_381_FR, O.BLS12_381_FR, 255), "bn254": (S.BN254_FR, O.BN254_FR, 254)}
# label: (field, rate, alpha, RF, RP)
CONFIGS = {
    "t3": ("bls", 2, 5, 8, 31),             # quad engine up to 32768 units, window t = 3 above: arity 2 only
    "t4": ("bls", 3, 5, 8, 56),
    "t5": ("bls", 4, 5, 8, 56),             # the reference's default parameters of rate 4 (the 4-ary fixture)
    "t6": ("bls", 5, 5, 8, 57),
    "t9-bn254": ("bn254", 8, 5, 8, 57),
    "t9-alpha17": ("bls", 8, 17, 8, 57),    # window t = 9 on the generic S-box
    "lds-t16": ("bls", 15, 5, 4, 6),        # run-time width
}


@functools.lru_cache(maxsize=None)
def config(label):
    """(product field, product config, C port)"""
    field, rate, alpha, rf, rp = CONFIGS[label]
    f, p, bits = FIELD[field]
    return f, S.poseidon_config_from_lfsr(f, rate, alpha, rf, rp), cref.CRef(O.make_config(p, bits, rate, alpha, rf, rp))


def shape(n_leaves, a):
    """(depth, n_nodes) by plain arithmetic"""
    depth, nodes, w = 0, n_leaves, n_leaves
    while w > 1:
        assert w % a == 0
        w //= a
        nodes += w
        depth += 1
    return depth, nodes


def forest(cr, leaves, n_trees, a):
    """level-major node array of n_trees trees over leaves [n_trees * m][4]: the C port's batch hash, level by level (a row of a
    children never straddles two trees: m is a power of a)"""
    levels = [np.ascontiguousarray(leaves, dtype=np.uint64).reshape(-1, 4)]
    while levels[-1].shape[0] > n_trees:
        levels.append(cr.hash_batch(levels[-1].reshape(-1, a, 4), a, 1, threads=0).reshape(-1, 4))
    return np.concatenate(levels)


def tree(cr, leaves, a):
    return forest(cr, leaves, 1, a)


@functools.lru_cache(maxsize=None)
def cached_tree(label, a, n_leaves, seed=0):
    """(leaves, nodes) of the tree every test of one case shares; read-only"""
    f, cfg, cr = config(label)
    leaves = synth.random_elements(f, n_leaves, seed=0xA51 + 1000 * a + n_leaves + seed)
    nodes = tree(cr, leaves, a)
    leaves.setflags(write=False)
    nodes.setflags(write=False)
    return leaves, nodes


def open_paths(nodes, n_leaves, a, indices):
    """[k][depth][a - 1][4] by the index arithmetic of the header, one sibling at a time"""
    depth, _ = shape(n_leaves, a)
    out = np.zeros((len(indices), depth, a - 1, 4), dtype=np.uint64)
    for i, index in enumerate(int(x) for x in indices):
        first, width, idx = 0, n_leaves, index
        for level in range(depth):
            digit, base = idx % a, first + idx - idx % a
            out[i, level] = [nodes[base + c] for c in range(a) if c != digit]
            first, width, idx = first + width, width // a, idx // a
    return out


def climb(cr, leaves, indices, paths, a):
    """hash leaves [k][4] up their paths: the running node goes back in at digit (index / a^level) % a.  Returns the k top nodes."""
    k, depth = paths.shape[0], paths.shape[1]
    cur = np.ascontiguousarray(leaves, dtype=np.uint64).reshape(k, 4).copy()
    idx = [int(x) for x in indices]
    for level in range(depth):
        rows = np.zeros((k, a, 4), dtype=np.uint64)
        for i in range(k):
            digit = (idx[i] // a ** level) % a
            rows[i, :digit] = paths[i, level, :digit]
            rows[i, digit] = cur[i]
            rows[i, digit + 1:] = paths[i, level, digit:]
        cur = cr.hash_batch(rows, a, 1, threads=0).reshape(k, 4)
    return cur


def path_indices(n_leaves, a, k, seed):
    """k leaf indices that include 0, n - 1 and - from a on - every digit value at the bottom level"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_leaves, k).astype(np.uint64)
    must = [0, n_leaves - 1] + [a * (j % max(n_leaves // a, 1)) + j for j in range(a)]
    for slot, value in enumerate(must[:k]):
        idx[slot] = min(value, n_leaves - 1)
    return idx
