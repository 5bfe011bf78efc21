"""Sequential leaf updates of a fixed-depth tree (pmx_merkle_update_witnesses) from the oracle's restatement in oracle/ (the C port behind
oracle/cref), for tests/test_merkle_chain_host.py and tests/test_gpu_merkle_witness.py.  Nothing here calls the product.

model() is the overlay model of include/poseidon_mi355x.h, written literally: one update at a time, one level at a time, one compression
of one row each.  sources() is the same walk without the hashing: which earlier update, if any, every sibling comes from; model_batched()
hashes level by level from sources() with the C port's batch hash, for a k the literal model takes too long over
(tests/test_merkle_chain_host.py asserts that the two agree).  sparse_tree() holds a tree nobody can pad as the nodes above its populated
leaves over the chain of default digests, and opens it."""
import numpy as np


def compress_one(cr, row, a):
    """the parent of one row [a][4]"""
    return cr.hash_batch(np.ascontiguousarray(row, dtype=np.uint64).reshape(1, a, 4), a, 1, threads=1).reshape(4)


def model(cr, a, depth, indices, new_leaves, paths):
    """(witness [k][depth][a - 1][4], roots [k][4]) by the overlay model"""
    k = len(indices)
    overlay = {}
    witness = np.zeros((k, depth, a - 1, 4), dtype=np.uint64)
    roots = np.zeros((k, 4), dtype=np.uint64)
    for j in range(k):
        index = int(indices[j])
        v = [np.array(new_leaves[j], dtype=np.uint64)]
        for l in range(depth):
            q = index // a ** l
            digit, base = q % a, q - q % a
            row = np.zeros((a, 4), dtype=np.uint64)
            for s, c in enumerate(c for c in range(a) if c != digit):
                witness[j, l, s] = overlay.get((l, base + c), paths[j][l][s])
                row[c] = witness[j, l, s]
            row[digit] = v[l]
            v.append(compress_one(cr, row, a))
        for l in range(depth + 1):
            overlay[(l, index // a ** l)] = v[l]
        roots[j] = v[depth]
    return witness, roots


def sources(a, depth, indices):
    """[depth][k][a - 1]: the update whose running node the sibling is, -1 for the caller's old opening"""
    k = len(indices)
    writer = {}
    out = [[[-1] * (a - 1) for _ in range(k)] for _ in range(depth)]
    for j in range(k):
        index = int(indices[j])
        for l in range(depth):
            q = index // a ** l
            digit, base = q % a, q - q % a
            for s, c in enumerate(c for c in range(a) if c != digit):
                out[l][j][s] = writer.get((l, base + c), -1)
        for l in range(depth + 1):
            writer[(l, index // a ** l)] = j
    return out


def model_batched(cr, a, depth, indices, new_leaves, paths):
    """model() level by level: the siblings picked by sources(), every level one batch hash of the C port"""
    k = len(indices)
    src = sources(a, depth, indices)
    paths = np.asarray(paths, dtype=np.uint64).reshape(k, depth, a - 1, 4)
    witness = np.zeros((k, depth, a - 1, 4), dtype=np.uint64)
    v = np.ascontiguousarray(new_leaves, dtype=np.uint64).reshape(k, 4)
    for l in range(depth):
        rows = np.zeros((k, a, 4), dtype=np.uint64)
        for j in range(k):
            digit = (int(indices[j]) // a ** l) % a
            for s, c in enumerate(c for c in range(a) if c != digit):
                witness[j, l, s] = v[src[l][j][s]] if src[l][j][s] >= 0 else paths[j, l, s]
                rows[j, c] = witness[j, l, s]
            rows[j, digit] = v[j]
        v = cr.hash_batch(rows, a, 1, threads=0).reshape(k, 4)
    return witness, v


def sparse_tree(cr, a, depth, e, leaves):
    """{(level, node): value} of the nodes above the populated leaves {index: leaf [4]}, every other position the default leaf e[0]"""
    nodes = {(0, int(i)): np.array(v, dtype=np.uint64) for i, v in leaves.items()}
    level = sorted(int(i) for i in leaves)
    for l in range(depth):
        parents = sorted({q // a for q in level})
        for p in parents:
            row = np.stack([nodes.get((l, p * a + c), np.asarray(e[l])) for c in range(a)])
            nodes[(l + 1, p)] = compress_one(cr, row, a)
        level = parents
    return nodes


def sparse_root(nodes, e, depth):
    return nodes.get((depth, 0), np.asarray(e[depth]))


def sparse_paths(nodes, a, depth, e, indices):
    """[k][depth][a - 1][4]: the openings of a sparse_tree; a sibling that is not held is an empty subtree, e[level]"""
    out = np.zeros((len(indices), depth, a - 1, 4), dtype=np.uint64)
    for i, index in enumerate(int(x) for x in indices):
        for l in range(depth):
            q = index // a ** l
            digit, base = q % a, q - q % a
            for s, c in enumerate(c for c in range(a) if c != digit):
                out[i, l, s] = nodes.get((l, base + c), e[l])
    return out
