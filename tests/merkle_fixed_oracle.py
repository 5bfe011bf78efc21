"""Trees of a fixed depth from the oracle's restatement in oracle/ (the C port behind oracle/cref), for tests/test_merkle_fixed_host.py and
tests/test_gpu_merkle_fixed.py.  Nothing here calls the product.  Configs and labels are those of tests/merkle_ary_oracle.py, plus a
width of 10 for the run-time-width engine.

The tree of arity a and depth D over n leaves is BY DEFINITION the tree of tests/merkle_ary_oracle.py over the leaf row padded with the
default leaf e[0] to a^D leaves: padded_levels does exactly that - it pads and hashes every level.  Everything the product returns is
read off those full levels: the dense array (level l's first max(1, ceil(n / a^l)) nodes), the frontier (per level the complete nodes
a floor(f / a) .. f - 1, f = floor(n / a^l), unused slots zero) and the root.  For depths nobody can pad (a^D up to 2^64)
sparse_levels hashes the populated part only, a short row filled up with the default digest of its level; that the two agree where
both exist is asserted in tests/test_merkle_fixed_host.py."""
import functools

import numpy as np

import sponge_amd as S
from sponge_amd import synth
from oracle import cref
from oracle import poseidon_oracle as O

import merkle_ary_oracle as M

CONFIGS = dict(M.CONFIGS)
CONFIGS["t10"] = ("bls", 9, 5, 4, 6)        # beyond the widths that have an engine of their own: the run-time-width engine


@functools.lru_cache(maxsize=None)
def config(label):
    """(product field, product config, C port)"""
    if label in M.CONFIGS:
        return M.config(label)
    field, rate, alpha, rf, rp = CONFIGS[label]
    f, p, bits = M.FIELD[field]
    return f, S.poseidon_config_from_lfsr(f, rate, alpha, rf, rp), cref.CRef(O.make_config(p, bits, rate, alpha, rf, rp))


def default_leaf(label):
    """a default leaf that is not zero: zero words are what an untouched buffer holds"""
    f, _, _ = config(label)
    return synth.random_elements(f, 1, seed=0xE0)[0]


def defaults(cr, e0, a, depth):
    """[depth + 1][4]: e[l + 1] = new; absorb(a copies of e[l]); squeeze_native(1)"""
    e = [np.ascontiguousarray(e0, dtype=np.uint64).reshape(4)]
    for _ in range(depth):
        e.append(cr.hash_batch(np.repeat(e[-1].reshape(1, 1, 4), a, axis=1), a, 1, threads=1).reshape(4))
    return np.stack(e)


@functools.lru_cache(maxsize=None)
def cached_defaults(label, a, depth):
    e = defaults(config(label)[2], default_leaf(label), a, depth)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def leaf_row(label, count, seed=0):
    """the leaves every test of a label appends, a prefix of one row; read-only"""
    leaves = synth.random_elements(config(label)[0], count, seed=0xF1ED + seed)
    leaves.setflags(write=False)
    return leaves


def padded_levels(cr, leaves, a, depth, e0):
    """the definition: pad with e[0] to a^depth leaves, hash every level; [depth + 1] arrays of a^(depth - l) nodes"""
    leaves = np.ascontiguousarray(leaves, dtype=np.uint64).reshape(-1, 4)
    row = np.empty((a ** depth, 4), dtype=np.uint64)
    row[:leaves.shape[0]] = leaves
    row[leaves.shape[0]:] = e0
    levels = [row]
    for _ in range(depth):
        levels.append(cr.hash_batch(levels[-1].reshape(-1, a, 4), a, 1, threads=0).reshape(-1, 4))
    return levels


def sparse_levels(cr, leaves, a, depth, e):
    """the populated part: level l's first ceil(n / a^l) nodes, a short row filled up with e[l]; n = 0: every level is empty"""
    levels = [np.ascontiguousarray(leaves, dtype=np.uint64).reshape(-1, 4)]
    for l in range(depth):
        cur = levels[-1]
        pad = -cur.shape[0] % a
        if pad:
            cur = np.concatenate([cur, np.repeat(np.asarray(e[l]).reshape(1, 4), pad, axis=0)])
        levels.append(cr.hash_batch(cur.reshape(-1, a, 4), a, 1, threads=0).reshape(-1, 4) if cur.shape[0] else cur)
    return levels


def root_of(levels, e, depth):
    return levels[depth][0] if levels[depth].shape[0] else np.asarray(e[depth])


def frontier_of(levels, n, a, depth):
    """[depth][a - 1][4]: per level the complete nodes a floor(f / a) .. f - 1, the other slots zero"""
    out = np.zeros((depth, a - 1, 4), dtype=np.uint64)
    for l in range(depth):
        f = n // a ** l
        out[l, :f % a] = levels[l][f - f % a:f]
    return out


def widths(n, a, depth):
    return [max(1, -(-n // a ** l)) for l in range(depth + 1)]


def dense_of(levels, n, a, depth):
    """the packed array of pmx_merkle_fixed: level l's first max(1, ceil(n / a^l)) nodes, leaves first, root last"""
    return np.concatenate([levels[l][:w] for l, w in enumerate(widths(n, a, depth))])


def open_paths(levels, n, a, depth, e, indices):
    """[k][depth][a - 1][4] off levels that hold at least the stored widths: a sibling beyond the stored width is e[level]"""
    w = widths(n, a, depth)
    out = np.zeros((len(indices), depth, a - 1, 4), dtype=np.uint64)
    for i, index in enumerate(int(x) for x in indices):
        assert index < n
        idx = index
        for level in range(depth):
            digit, base = idx % a, idx - idx % a
            for s, c in enumerate(c for c in range(a) if c != digit):
                out[i, level, s] = levels[level][base + c] if base + c < w[level] else e[level]
            idx //= a
    return out


@functools.lru_cache(maxsize=None)
def cached_padded(label, a, depth, n):
    """the full levels of the tree over the first n leaves of the label's row"""
    levels = padded_levels(config(label)[2], leaf_row(label, a ** depth)[:n], a, depth, default_leaf(label))
    for level in levels:
        level.setflags(write=False)
    return levels
