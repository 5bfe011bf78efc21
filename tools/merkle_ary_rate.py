"""The 8-ary Merkle tree of BN254 Fr t = 9 (rate 8) over 2^21 leaves, device-resident, three ways in one process, alternating:
  ary     pmx_merkle_ary_dev(arity 8)                                      - compress_ary_kernel, 7 launches
  loop    pmx_hash_batch_dev(in_len 8, out_len 1) over the 7 levels         - what a caller could do before: hash_kernel, 7 launches
  2to1    pmx_merkle_2to1_dev over the same leaves                         - 21 launches, 7 x the permutations
Every step is timed by HIP events on the launch stream (the leaves stay in place: a tree only writes behind them); each round runs the
three forms once, in this order, after a warm-up round.  Reported per form: median, min, max and the spread (max - min) / median of its
own repeated runs.  Before timing, `ary` and `loop` must agree on every node, and `ary` with oracle/cref on every node.
Prints one JSON line.   usage: python tools/merkle_ary_rate.py [--rounds 30] [--log2-leaves 21]"""
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
from sponge_amd import _lib, synth  # noqa: E402
from oracle import cref  # noqa: E402
from oracle import poseidon_oracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--log2-leaves", type=int, default=21, help="a multiple of 3 (the leaves are a power of 8)")
ARGS = ap.parse_args()
assert ARGS.log2_leaves % 3 == 0
DEV = torch.device("cuda", 0)
WARMUP = 3
A = 8


def main():
    cfg = S.poseidon_config_from_lfsr(S.BN254_FR, 8, 5, 8, 57)
    ctx, m = cfg.context(0), 1 << ARGS.log2_leaves
    st = torch.cuda.current_stream().cuda_stream
    widths = [m]
    while widths[-1] > 1:
        widths.append(widths[-1] // A)
    n_ary, n_two = sum(widths), 2 * m - 1
    leaves = synth.random_elements(S.BN254_FR, m, seed=0xA8)
    d_leaves = torch.from_numpy(leaves.view(np.int64)).to(DEV)
    d_ary = torch.zeros((n_ary, 4), dtype=torch.int64, device=DEV)
    d_loop = torch.zeros((n_ary, 4), dtype=torch.int64, device=DEV)
    d_two = torch.zeros((n_two, 4), dtype=torch.int64, device=DEV)
    for d in (d_ary, d_loop, d_two):
        d[:m].copy_(d_leaves)

    def ary():
        ctx.merkle_ary_dev(d_ary.data_ptr(), m, A, st)

    def loop():
        src = 0
        for w in widths[:-1]:
            ctx.hash_batch_dev(d_loop.data_ptr() + src * 32, A, d_loop.data_ptr() + (src + w) * 32, 1, w // A, st)
            src += w

    def two():
        ctx.merkle_2to1_dev(d_two.data_ptr(), m, st)

    forms = [("ary", ary), ("loop", loop), ("2to1", two)]
    for _, fn in forms:
        fn()
    torch.cuda.synchronize()
    got = d_ary.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, d_loop.cpu().numpy().view(np.uint64)), "pmx_merkle_ary_dev and the hash loop disagree"
    cr = cref.CRef(O.make_config(O.BN254_FR, 254, 8, 5, 8, 57))
    src = 0
    for w in widths[:-1]:
        want = cr.hash_batch(got[src:src + w].reshape(-1, A, 4), A, 1, threads=0).reshape(-1, 4)
        assert np.array_equal(got[src + w:src + w + w // A], want), "level of %d parents differs from the oracle" % (w // A)
        src += w

    stream = torch.cuda.current_stream()
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

    def stats(xs):
        med = float(np.median(xs))
        return {"median_ms": round(med, 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
                "spread_over_median": round((max(xs) - min(xs)) / med, 4)}

    out = {"tool": "merkle_ary_rate", "config": "bn254_fr t=9 a=5 8/57", "arity": A, "leaves": m, "rounds": ARGS.rounds, "warmup": WARMUP,
           "device": torch.cuda.get_device_name(0), "levels": {"ary": len(widths) - 1, "2to1": ARGS.log2_leaves},
           "permutations": {"ary": (m - 1) // (A - 1), "2to1": m - 1},
           "checked": "every node: ary == loop == oracle/cref"}
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        out["clocks"] = [ln.strip() for ln in smi.splitlines() if "sclk" in ln or "mclk" in ln][:2]   # (read-only query)
    except Exception as e:   # the tool is optional on a box without it
        out["clocks"] = "unavailable: %s" % type(e).__name__
    for name, _ in forms:
        out[name] = stats(times[name])
    out["ary_over_loop"] = round(out["ary"]["median_ms"] / out["loop"]["median_ms"], 4)
    out["2to1_over_ary"] = round(out["2to1"]["median_ms"] / out["ary"]["median_ms"], 3)
    info = _lib.PmxEngineInfo()
    import ctypes
    _lib.check(_lib.lib().pmx_ctx_engine_info(ctx._h, _lib.OP_COMPRESS, m // A, A, ctypes.byref(info)))
    out["engine"] = info.engine.decode()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
