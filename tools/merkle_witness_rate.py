"""k = 2^14 sequential leaf updates of a fixed-depth tree with witnesses (pmx_merkle_update_witnesses), host buffers, beside their floor:
  call        the whole call through the C ABI, pageable numpy buffers touched before: the plan, `depth` slabs up, `depth` gathers and
              compressions, witnesses and roots down
  no_witness  the same call with witness_out = NULL: nothing of the openings comes back
  floor       `depth` launches of launch_compress_ary over k rows alone, device-resident - pmx_merkle_ary_forest_dev over k trees of
              `arity` leaves is exactly one such launch -, timed by HIP events on the launch stream (this form needs nothing the new
              entry adds: it runs unchanged on the commit before it)
for (arity 2, depth 32) at BLS12-381 Fr t = 3 and (arity 8, depth 11) at BN254 Fr t = 9.  The old tree is the empty one: every sibling of
the old openings is a default digest.  Half the indices lie among 4 k leaves at the low end (shared ancestors, repeats), half anywhere.
call and no_witness are wall-clock times around the synchronous call.  Per form: median, min, max, spread of its repeated runs; then
floor_over_call (the launches' share), and (call - no_witness) / call (the witness download's share).
Prints one JSON line.   usage: python tools/merkle_witness_rate.py [--rounds 20] [--log2-k 14]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sponge_amd as S  # noqa: E402
from sponge_amd import _lib, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--log2-k", type=int, default=14)
ARGS = ap.parse_args()
DEV = torch.device("cuda", 0)
WARMUP = 3
CASES = [("bls12_381_fr t=3 a=5 8/31", S.BLS12_381_FR, (2, 5, 8, 31), 2, 32), ("bn254_fr t=9 a=5 8/57", S.BN254_FR, (8, 5, 8, 57), 8, 11)]


def stats(xs):
    med = float(np.median(xs))
    return {"median_ms": round(med, 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "spread_over_median": round((max(xs) - min(xs)) / med, 4)}


def main():
    k = 1 << ARGS.log2_k
    out = {"tool": "merkle_witness_rate", "k": k, "rounds": ARGS.rounds, "warmup": WARMUP, "device": torch.cuda.get_device_name(0), "cases": {}}
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        out["clocks"] = [ln.strip() for ln in smi.splitlines() if "sclk" in ln or "mclk" in ln][:2]   # (read-only query)
    except Exception as e:   # the tool is optional on a box without it
        out["clocks"] = "unavailable: %s" % type(e).__name__
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    for name, field, (rate, alpha, rf, rp), a, depth in CASES:
        ctx = S.poseidon_config_from_lfsr(field, rate, alpha, rf, rp).context(0)
        cap = a ** depth
        rng = np.random.default_rng(k + a)
        idx = np.where(np.arange(k) % 2 == 0, rng.integers(0, 4 * k, k), rng.integers(0, cap, k)).astype(np.uint64)
        new = synth.random_elements(field, k, seed=0xB0 + a)
        e = ctx.merkle_fixed_defaults(np.zeros(4, dtype=np.uint64), a, depth)
        paths = np.ascontiguousarray(np.broadcast_to(e[:depth].reshape(1, depth, 1, 4), (k, depth, a - 1, 4)))
        d_rows = torch.zeros((k * (a + 1), 4), dtype=torch.int64, device=DEV)       # k trees of `a` leaves, level-major: leaves, then roots
        d_rows[:k * a].copy_(torch.from_numpy(synth.random_elements(field, k * a, seed=7).view(np.int64)))

        # (the C ABI on buffers allocated and touched once: a call pays for no fresh pages)
        wit, roots, roots2 = np.ones((k, depth, a - 1, 4), dtype=np.uint64), np.ones((k, 4), dtype=np.uint64), np.ones((k, 4), dtype=np.uint64)
        fn_c, ptr = _lib.lib().pmx_merkle_update_witnesses, lambda x: ctypes.c_void_p(x.ctypes.data)

        def call():
            _lib.check(fn_c(ctx._h, a, depth, ptr(idx), ptr(new), ptr(paths), k, ptr(wit), ptr(roots), None))

        def no_witness():
            _lib.check(fn_c(ctx._h, a, depth, ptr(idx), ptr(new), ptr(paths), k, None, ptr(roots2), None))

        def floor():
            for _ in range(depth):
                ctx.merkle_ary_forest_dev(d_rows.data_ptr(), k, a, a, st)

        call()
        no_witness()
        assert np.array_equal(roots, roots2) and np.array_equal(wit[0], paths[0]) and not np.array_equal(roots[0], roots[1])
        times = {"call": [], "no_witness": [], "floor": []}
        for r in range(WARMUP + ARGS.rounds):
            for form, fn in (("call", call), ("no_witness", no_witness)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if r >= WARMUP:
                    times[form].append((time.perf_counter() - t0) * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            floor()
            e1.record(stream)
            e1.synchronize()
            if r >= WARMUP:
                times["floor"].append(e0.elapsed_time(e1))
        rec = {form: stats(xs) for form, xs in times.items()}
        rec.update(arity=a, depth=depth, permutations=k * depth, opening_mib=round(paths.nbytes / 2 ** 20, 2),
                   floor_over_call=round(rec["floor"]["median_ms"] / rec["call"]["median_ms"], 4),
                   witness_download_share=round((rec["call"]["median_ms"] - rec["no_witness"]["median_ms"]) / rec["call"]["median_ms"], 4))
        out["cases"][name] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
