"""Trees of a fixed depth (pmx_merkle_frontier_append, pmx_merkle_fixed) through their host-buffer entries, every comparison inside one
process, on (k = 2, D = 32, BLS12-381 Fr t = 3) and (k = 8, D = 21, BN254 Fr t = 9):
  append   pmx_merkle_frontier_append of m = 2^10, 2^16, 2^20 leaves to the empty tree against what the library offered before,
           pmx_merkle_ragged (root only) over the same m leaves - a tree of the same permutation count to within D.  "top_share": the
           D - ceil(log_k m) levels above the populated part are launches of ONE unit; their share of the append is estimated from an
           append of a single leaf, whose D launches are all of that kind: (time of that append / D) * (D - ceil(log_k m)) / time.
  dense    where a dense tree fits (k = 2, D = 20 and k = 8, D = 7): pmx_merkle_fixed (root only) over n = 2^10 and n = k^D leaves against
           the only earlier route to the SAME root, pmx_merkle_ary over the row padded to k^D leaves (the padding itself is not timed).
  pieces   the piece bound of the walk in powers of two (pmx_test_merkle_fixed_piece of the test library, so every size runs through the
           product's own host loop) on an append of 2^22 leaves; per size the median and the spread (max - min) / median.
Host wall-clock around calls that return after their last download; medians of --rounds runs after one warm-up, the forms of a comparison
alternating inside every round.  Before timing, every append's root is compared with the tree pmx_merkle_ragged builds where the two
definitions meet (m = k^j: the populated subtree's root hashed up over the default chain by the C port).
Prints one JSON line per measurement.   usage: python tools/merkle_fixed_rate.py [--rounds 5] [--skip-pieces]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sponge_amd import _lib  # noqa: E402

_lib.use_test_library()          # the shipped objects + the piece hook
import sponge_amd as S  # noqa: E402
from sponge_amd import synth  # noqa: E402
from oracle import cref  # noqa: E402
from oracle import poseidon_oracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--skip-pieces", action="store_true")
ARGS = ap.parse_args()

CONFIGS = [
    ("bls12_381_fr t=3", S.BLS12_381_FR, O.BLS12_381_FR, 255, (2, 5, 8, 31), 2, 32, 20),
    ("bn254_fr t=9", S.BN254_FR, O.BN254_FR, 254, (8, 5, 8, 57), 8, 21, 7),
]


def timed(forms, rounds):
    times = {name: [] for name, _ in forms}
    for r in range(1 + rounds):
        for name, fn in forms:
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r:
                times[name].append(dt)
    return {name: {"median_ms": round(float(np.median(xs)), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
                   "spread_over_median": round((max(xs) - min(xs)) / float(np.median(xs)), 4)} for name, xs in times.items()}


def emit(rec):
    print(json.dumps(rec), flush=True)


def main():
    for name, f, p, bits, (rate, alpha, rf, rp), k, depth, dense_depth in CONFIGS:
        cfg = S.poseidon_config_from_lfsr(f, rate, alpha, rf, rp)
        ctx = cfg.context(0)
        cr = cref.CRef(O.make_config(p, bits, rate, alpha, rf, rp))
        e0 = synth.random_elements(f, 1, seed=0xE0)[0]
        e = ctx.merkle_fixed_defaults(e0, k, depth)
        leaves = synth.random_elements(f, 1 << 22, seed=0xF1)
        one = timed([("append1", lambda: ctx.merkle_frontier_append(k, depth, e, None, 0, leaves[:1]))], ARGS.rounds)["append1"]
        for log2m in (10, 16, 20):
            m = 1 << log2m
            row = leaves[:m]
            levels = -(-log2m // int(np.log2(k)))                   # ceil(log_k m)
            # where the definitions meet: m = k^levels leaves fill a subtree whose root pmx_merkle_ragged gives; above it, default siblings
            _, root = ctx.merkle_frontier_append(k, depth, e, None, 0, row)
            if k ** levels == m:
                _, top = ctx.merkle_ragged(row, k, want_nodes=False)
                for l in range(levels, depth):
                    top = cr.hash_batch(np.concatenate([top.reshape(1, 4), np.repeat(e[l].reshape(1, 4), k - 1, axis=0)]).reshape(1, k, 4), k, 1, threads=1).reshape(4)
                assert np.array_equal(root, top), "append root differs from ragged subtree + default chain"
            res = timed([("append", lambda: ctx.merkle_frontier_append(k, depth, e, None, 0, row)),
                         ("ragged", lambda: ctx.merkle_ragged(row, k, want_nodes=False))], ARGS.rounds)
            top_levels = depth - levels
            emit({"tool": "merkle_fixed_rate", "what": "append", "config": name, "arity": k, "depth": depth, "m": m, **res,
                  "append_over_ragged": round(res["append"]["median_ms"] / res["ragged"]["median_ms"], 4),
                  "single_leaf_append_ms": one["median_ms"], "single_unit_top_levels": top_levels,
                  "top_share": round(one["median_ms"] / depth * top_levels / res["append"]["median_ms"], 4)})
        # the dense comparison: the same root two ways
        d = dense_depth
        ed = ctx.merkle_fixed_defaults(e0, k, d)
        cap = k ** d
        for n in (1 << 10, cap):
            padded = np.empty((cap, 4), dtype=np.uint64)
            padded[:n] = leaves[:n]
            padded[n:] = e0
            row = leaves[:n]
            _, a = ctx.merkle_fixed(row, k, d, ed, want_nodes=False)
            _, b = ctx.merkle_ary(padded, k, want_nodes=False)
            assert a.tobytes() == b.tobytes(), "pmx_merkle_fixed and pmx_merkle_ary over the padded row disagree"
            res = timed([("fixed", lambda: ctx.merkle_fixed(row, k, d, ed, want_nodes=False)),
                         ("ary_padded", lambda: ctx.merkle_ary(padded, k, want_nodes=False))], ARGS.rounds)
            emit({"tool": "merkle_fixed_rate", "what": "dense", "config": name, "arity": k, "depth": d, "n": n, "positions": cap, **res,
                  "ary_padded_over_fixed": round(res["ary_padded"]["median_ms"] / res["fixed"]["median_ms"], 3)})
        if ARGS.skip_pieces:
            continue
        m = 1 << 22
        hook = _lib.lib().pmx_test_merkle_fixed_piece
        want = None
        for log2p in range(14, 23):
            hook(1 << log2p)
            got, root = ctx.merkle_frontier_append(k, depth, e, None, 0, leaves)
            want = want if want is not None else (got.tobytes(), root.tobytes())
            assert (got.tobytes(), root.tobytes()) == want, "pieces changed a byte"
            res = timed([("append", lambda: ctx.merkle_frontier_append(k, depth, e, None, 0, leaves))], ARGS.rounds)["append"]
            emit({"tool": "merkle_fixed_rate", "what": "pieces", "config": name, "arity": k, "depth": depth, "m": m, "piece": 1 << log2p, **res})
        hook(0)


if __name__ == "__main__":
    main()
