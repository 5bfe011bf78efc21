#!/usr/bin/env python3
"""Regenerates tests/golden/merkle_ragged_vectors.json.  Run from the repo root:  python tests/golden/make_merkle_ragged_golden.py

Every node of two trees whose leaf count is no power of the arity, from the KAT-pinned Python big-integer oracle
(oracle/poseidon_oracle.py) alone - the C port (oracle/poseidon_ref.c) and the product take no part, so the fixture pins both:
  * a 4-ary tree of 6 leaves on the reference's default parameters of rate 4 for BLS12-381 Fr (alpha 5, 8 + 56 rounds, t = 5):
    levels of 6, 2, 1 nodes - a short parent of 2 children, then a top parent of 2,
  * an 8-ary tree of 9 leaves on bn254_t9_a5_8_57 (BN254 Fr, rate 8: the benchmarked t = 9 config): levels of 9, 2, 1 - a short parent
    of ONE child (a permutation, not a promotion), then a top parent of 2.
Level l + 1 has ceil(M_l / arity) nodes; a parent is (new; absorb(the children that exist); squeeze_native_field_elements(1))[0]
(src/poseidon/mod.rs:126-135, 219-230, 324-328) - the short one absorbs r < arity elements, nothing is padded.
nodes: the leaves, then every level, root last.  All integers are canonical field values written as hex strings."""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import poseidon_oracle as O  # noqa: E402

# name -> (field name, p, prime_bits, rate, alpha, RF, RP, arity, leaves)
TREES = {
    "bls_t5_a5_8_56/arity4/leaves6": ("bls12_381_fr", O.BLS12_381_FR, 255, 4, 5, 8, 56, 4, 6),
    "bn254_t9_a5_8_57/arity8/leaves9": ("bn254_fr", O.BN254_FR, 254, 8, 5, 8, 57, 8, 9),
}


def tree_nodes(cfg, leaves, arity):
    nodes, level = list(leaves), list(leaves)
    while len(level) > 1:
        level = [O.hash_fixed(cfg, level[i:i + arity], 1)[0] for i in range(0, len(level), arity)]      # (the last slice may be short)
        nodes += level
    return nodes


def main():
    out = {}
    for name, (fname, p, bits, rate, alpha, rf, rp, arity, m) in TREES.items():
        cfg = O.make_config(p, bits, rate, alpha, rf, rp)
        rng = random.Random("merkle_ragged/" + name)
        leaves = [rng.randrange(p) for _ in range(m)]
        leaves[0], leaves[1], leaves[m - 1] = 0, p - 1, 1      # edge values in the first parent and in the short one
        out[name] = {"field": fname, "prime_bits": bits, "rate": rate, "alpha": alpha, "full_rounds": rf, "partial_rounds": rp,
                     "arity": arity, "n_leaves": m, "nodes": [hex(v) for v in tree_nodes(cfg, leaves, arity)]}
    path = os.path.join(HERE, "merkle_ragged_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
