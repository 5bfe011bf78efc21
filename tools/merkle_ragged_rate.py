"""Trees over any number of leaves (pmx_merkle_ragged_dev) on BN254 Fr t = 9 (rate 8), device-resident, two comparisons in one process:
  (a) a power of the arity, 2^21 leaves at arity 8:   ragged   pmx_merkle_ragged_dev      against   ary    pmx_merkle_ary_dev
      - the same launches by construction (every level divides); the ragged entry may be slower by no more than ary's own spread.
  (b) the case the entries exist for, 2^20 leaves:    ragged8  pmx_merkle_ragged_dev(8)   against   2to1   pmx_merkle_2to1_dev
      - 149 797 permutations in 7 levels (the top parent has 4 children) against 1 048 575 in 20: 7.0 x by permutation count.
Every step is timed by HIP events on the launch stream (the leaves stay in place: a tree only writes behind them); the forms of a
comparison alternate inside every round, after warm-up rounds.  Reported per form: median, min, max and the spread (max - min) / median of
its own repeated runs.  Before timing every node of every form is compared with oracle/cref (the short parent as an absorb of the children
that exist), and ragged with ary byte for byte.
Prints one JSON line.   usage: python tools/merkle_ragged_rate.py [--rounds 30]"""
import argparse
import ctypes
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
from sponge_amd.poseidon import merkle_ragged_shape  # noqa: E402
from oracle import cref  # noqa: E402
from oracle import poseidon_oracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--log2-power", type=int, default=21, help="comparison (a): a multiple of 3")
ap.add_argument("--log2-ragged", type=int, default=20, help="comparison (b): any")
ARGS = ap.parse_args()
assert ARGS.log2_power % 3 == 0
DEV = torch.device("cuda", 0)
WARMUP = 3
A = 8


def check_against_oracle(cr, got, m, a):
    """every level of the node array `got` from the level below it, by the C port"""
    src, w = 0, m
    while w > 1:
        full, r = divmod(w, a)
        level = got[src:src + w]
        want = [cr.hash_batch(level[:full * a].reshape(full, a, 4), a, 1, threads=0).reshape(full, 4)] if full else []
        if r:
            want.append(cr.hash_batch(level[full * a:].reshape(1, r, 4), r, 1, threads=0).reshape(1, 4))
        want = np.concatenate(want)
        assert np.array_equal(got[src + w:src + w + want.shape[0]], want), "level of %d parents (arity %d) differs from the oracle" % (want.shape[0], a)
        src, w = src + w, want.shape[0]
    assert src + 1 == got.shape[0]


def timed(forms, rounds):
    stream = torch.cuda.current_stream()
    times = {name: [] for name, _ in forms}
    for r in range(WARMUP + rounds):
        for name, fn in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r >= WARMUP:
                times[name].append(e0.elapsed_time(e1))
    out = {}
    for name, xs in times.items():
        med = float(np.median(xs))
        out[name] = {"median_ms": round(med, 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
                     "spread_over_median": round((max(xs) - min(xs)) / med, 4)}
    return out


def main():
    cfg = S.poseidon_config_from_lfsr(S.BN254_FR, 8, 5, 8, 57)
    ctx = cfg.context(0)
    cr = cref.CRef(O.make_config(O.BN254_FR, 254, 8, 5, 8, 57))
    st = torch.cuda.current_stream().cuda_stream
    out = {"tool": "merkle_ragged_rate", "config": "bn254_fr t=9 a=5 8/57", "rounds": ARGS.rounds, "warmup": WARMUP,
           "device": torch.cuda.get_device_name(0)}
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        out["clocks"] = [ln.strip() for ln in smi.splitlines() if "sclk" in ln or "mclk" in ln][:2]   # (read-only query)
    except Exception as e:   # the tool is optional on a box without it
        out["clocks"] = "unavailable: %s" % type(e).__name__

    def image(n_nodes, d_leaves, m):
        d = torch.zeros((n_nodes, 4), dtype=torch.int64, device=DEV)
        d[:m].copy_(d_leaves)
        return d

    # (a) a power of the arity
    m = 1 << ARGS.log2_power
    depth, n_nodes = merkle_ragged_shape(m, A)
    leaves = synth.random_elements(S.BN254_FR, m, seed=0xA8)
    d_leaves = torch.from_numpy(leaves.view(np.int64)).to(DEV)
    d_rag, d_ary = image(n_nodes, d_leaves, m), image(n_nodes, d_leaves, m)
    forms = [("ragged", lambda: ctx.merkle_ragged_dev(d_rag.data_ptr(), m, A, st)), ("ary", lambda: ctx.merkle_ary_dev(d_ary.data_ptr(), m, A, st))]
    for _, fn in forms:
        fn()
    torch.cuda.synchronize()
    got = d_rag.cpu().numpy().view(np.uint64)
    assert got.tobytes() == d_ary.cpu().numpy().tobytes(), "pmx_merkle_ragged_dev and pmx_merkle_ary_dev disagree"
    check_against_oracle(cr, got, m, A)
    a_res = timed(forms, ARGS.rounds)
    a_res.update({"leaves": m, "levels": depth, "permutations": n_nodes - m,
                  "ragged_over_ary": round(a_res["ragged"]["median_ms"] / a_res["ary"]["median_ms"], 4)})
    a_res["within_ary_spread"] = bool(a_res["ragged"]["median_ms"] - a_res["ary"]["median_ms"] <= a_res["ary"]["max_ms"] - a_res["ary"]["min_ms"])
    out["power_of_arity"] = a_res
    del d_rag, d_ary, d_leaves

    # (b) 2^k leaves that are no power of 8
    m = 1 << ARGS.log2_ragged
    depth, n_nodes = merkle_ragged_shape(m, A)
    leaves = synth.random_elements(S.BN254_FR, m, seed=0xA9)
    d_leaves = torch.from_numpy(leaves.view(np.int64)).to(DEV)
    d_rag, d_two = image(n_nodes, d_leaves, m), image(2 * m - 1, d_leaves, m)
    forms = [("ragged8", lambda: ctx.merkle_ragged_dev(d_rag.data_ptr(), m, A, st)), ("2to1", lambda: ctx.merkle_2to1_dev(d_two.data_ptr(), m, st))]
    for _, fn in forms:
        fn()
    torch.cuda.synchronize()
    check_against_oracle(cr, d_rag.cpu().numpy().view(np.uint64), m, A)
    check_against_oracle(cr, d_two.cpu().numpy().view(np.uint64), m, 2)
    b_res = timed(forms, ARGS.rounds)
    b_res.update({"leaves": m, "levels": {"ragged8": depth, "2to1": ARGS.log2_ragged}, "permutations": {"ragged8": n_nodes - m, "2to1": m - 1},
                  "by_permutation_count": round((m - 1) / (n_nodes - m), 3),
                  "2to1_over_ragged8": round(b_res["2to1"]["median_ms"] / b_res["ragged8"]["median_ms"], 3)})
    out["ragged"] = b_res
    out["checked"] = "every node of every form == oracle/cref; ragged == ary byte for byte"
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(ctx._h, _lib.OP_COMPRESS, m // A, A, ctypes.byref(info)))
    out["engine"] = info.engine.decode()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
