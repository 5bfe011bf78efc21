"""k leaves of the 8-ary Merkle tree of BN254 Fr t = 9 (rate 8) over 2^21 leaves change, device-resident, two ways in one process:
  update   pmx_merkle_ary_update_dev(k updates) on the resident tree     - at most k * 7 permutations: gather, compress, scatter per level
  rebuild  pmx_merkle_ary_dev over the leaf row with the updates in place - 299 593 permutations, what a caller had to do before
for k = 1, 64, 1024, 65536.  Every step is timed by HIP events on the launch stream; each round runs the two forms once, in this order,
after warm-up rounds (the update writes the same leaves again: the same work every round).  Reported per form: median, min, max and the
spread (max - min) / median of its own repeated runs, and rebuild_over_update.  Before timing, for every k, the updated tree must equal
the rebuilt one on every node, and the rebuilt one oracle/cref on every node.
Prints one JSON line.   usage: python tools/merkle_update_rate.py [--rounds 30] [--log2-leaves 21] [--k 1,64,1024,65536]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sponge_amd as S  # noqa: E402
from sponge_amd import synth  # noqa: E402
from oracle import cref  # noqa: E402
from oracle import poseidon_oracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--log2-leaves", type=int, default=21, help="a multiple of 3 (the leaves are a power of 8)")
ap.add_argument("--k", default="1,64,1024,65536")
ARGS = ap.parse_args()
assert ARGS.log2_leaves % 3 == 0
DEV = torch.device("cuda", 0)
WARMUP = 3
A = 8


def stats(xs):
    med = float(np.median(xs))
    return {"median_ms": round(med, 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "spread_over_median": round((max(xs) - min(xs)) / med, 4)}


def main():
    cfg = S.poseidon_config_from_lfsr(S.BN254_FR, 8, 5, 8, 57)
    cr = cref.CRef(O.make_config(O.BN254_FR, 254, 8, 5, 8, 57))
    ctx, m = cfg.context(0), 1 << ARGS.log2_leaves
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    widths = [m]
    while widths[-1] > 1:
        widths.append(widths[-1] // A)
    n_nodes, depth = sum(widths), len(widths) - 1
    leaves = synth.random_elements(S.BN254_FR, m, seed=0xA8)
    d_old = torch.zeros((n_nodes, 4), dtype=torch.int64, device=DEV)
    d_old[:m].copy_(torch.from_numpy(leaves.view(np.int64)))
    ctx.merkle_ary_dev(d_old.data_ptr(), m, A, st)
    d_tree, d_rebuild = d_old.clone(), d_old.clone()

    out = {"tool": "merkle_update_rate", "config": "bn254_fr t=9 a=5 8/57", "arity": A, "leaves": m, "rounds": ARGS.rounds, "warmup": WARMUP,
           "device": torch.cuda.get_device_name(0), "levels": depth, "rebuild_permutations": (m - 1) // (A - 1),
           "checked": "every node, every k: update == rebuild == oracle/cref", "k": {}}
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        out["clocks"] = [ln.strip() for ln in smi.splitlines() if "sclk" in ln or "mclk" in ln][:2]   # (read-only query)
    except Exception as e:   # the tool is optional on a box without it
        out["clocks"] = "unavailable: %s" % type(e).__name__

    for k in [int(x) for x in ARGS.k.split(",")]:
        assert 1 <= k <= m
        rng = np.random.default_rng(k)
        idx = rng.choice(m, k, replace=False).astype(np.uint64)
        new = synth.random_elements(S.BN254_FR, k, seed=0xB0 + k)
        d_idx = torch.from_numpy(idx.view(np.int64)).to(DEV)
        d_new = torch.from_numpy(new.view(np.int64)).to(DEV)
        d_work = torch.zeros(k * (A + 1) * 4, dtype=torch.int64, device=DEV)
        d_tree.copy_(d_old)
        d_rebuild[:m].copy_(d_old[:m])
        d_rebuild[d_idx] = d_new.reshape(k, 4)

        def update():
            ctx.merkle_ary_update_dev(d_tree.data_ptr(), m, A, d_idx.data_ptr(), d_new.data_ptr(), k, d_work.data_ptr(), st)

        def rebuild():
            ctx.merkle_ary_dev(d_rebuild.data_ptr(), m, A, st)

        forms = [("update", update), ("rebuild", rebuild)]
        for _, fn in forms:
            fn()
        torch.cuda.synchronize()
        got = d_rebuild.cpu().numpy().view(np.uint64)
        assert np.array_equal(d_tree.cpu().numpy().view(np.uint64), got), "k = %d: the updated tree is not the rebuilt one" % k
        after = leaves.copy()
        after[idx.astype(np.int64)] = new
        assert np.array_equal(got[:m], after)
        src = 0
        for w in widths[:-1]:
            want = cr.hash_batch(got[src:src + w].reshape(-1, A, 4), A, 1, threads=0).reshape(-1, 4)
            assert np.array_equal(got[src + w:src + w + w // A], want), "k = %d: level of %d parents differs from the oracle" % (k, w // A)
            src += w

        times = {name: [] for name, _ in forms}
        for r in range(WARMUP + ARGS.rounds):
            for name, fn in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if r >= WARMUP:
                    times[name].append(e0.elapsed_time(e1))
        # the permutations the update ran: k per gathered level, the level's width from the first level with k >= width on
        perms, w = 0, m
        for _ in range(depth):
            w //= A
            perms += k if k < w else w
        rec = {name: stats(times[name]) for name, _ in forms}
        rec["update_permutations"] = perms
        rec["rebuild_over_update"] = round(rec["rebuild"]["median_ms"] / rec["update"]["median_ms"], 3)
        out["k"][str(k)] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
