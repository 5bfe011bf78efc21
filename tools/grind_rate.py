#!/usr/bin/env python3
"""Rates of pmx_sponge_grind on the device, for profiles/grind/README.md.

  sweep   time to the answer for bits = 16, 20, 24 against chunk sizes 2^16 .. 2^24 (t = 3 BLS12-381 Fr): the chunk goes through the test
          library's hook (pmx_test_grind_chunk), so every size runs the product's own host loop; the nonce that comes back is the same
          for every chunk size, or the run stops.
  long    candidates/s of a search that finds nothing (bits = 60) over `units` candidates at the chosen chunk, for t = 3 BLS and t = 9
          BN254, next to the permutations/s of pmx_permute_batch_dev over the same number of units (resident states, events around
          `reps` launches), in the same process.
usage: grind_rate.py [sweep] [long] [--reps R] [--units-log2 L]      one JSON line per measurement"""
import argparse
import ctypes
import json
import sys
import time
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import sponge_amd as S  # noqa: E402
from sponge_amd import _lib, synth  # noqa: E402

CONFIGS = {"t3-bls": (S.BLS12_381_FR, 2, 5, 8, 31), "t9-bn254": (S.BN254_FR, 8, 5, 8, 57)}


def setup(label):
    f, rate, alpha, rf, rp = CONFIGS[label]
    cfg = S.poseidon_config_from_lfsr(f, rate, alpha, rf, rp)
    state = synth.random_elements(f, cfg.t, seed=0x6121D).reshape(cfg.t, 4)
    return cfg, cfg.context(0), state


def engine(ctx, op, n):
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(ctx._h, op, n, 0, ctypes.byref(info)))
    return info.engine.decode()


def timed_grind(ctx, state, bits, first, count):
    t0 = time.perf_counter()
    got = ctx.sponge_grind(state, _lib.MODE_ABSORBING, 0, bits, first, count)
    return got, time.perf_counter() - t0


def sweep(reps):
    cfg, ctx, state = setup("t3-bls")
    lib = _lib.lib()
    ctx.sponge_grind(state, 0, 0, 8, 0, 1 << 12)   # warm-up: module load, staging
    for bits in (16, 20, 24):
        answers = set()
        for log2 in range(16, 25):
            _lib.check(lib.pmx_test_grind_chunk(1 << log2))
            times = []
            for _ in range(reps):
                got, dt = timed_grind(ctx, state, bits, 0, None)
                times.append(dt)
                answers.add(got)
            assert len(answers) == 1, ("the answer depends on the chunk size", bits, log2, answers)
            nonce = got
            print(json.dumps({"what": "sweep", "bits": bits, "chunk_log2": log2, "nonce": nonce, "launches": nonce // (1 << log2) + 1,
                              "ms_median": round(1e3 * sorted(times)[len(times) // 2], 3), "ms_min": round(1e3 * min(times), 3),
                              "engine": engine(ctx, _lib.OP_GRIND, 1 << log2)}), flush=True)
    _lib.check(lib.pmx_test_grind_chunk(0))


def long_search(reps, units_log2):
    import torch
    units = 1 << units_log2
    for label in CONFIGS:
        cfg, ctx, state = setup(label)
        ctx.sponge_grind(state, 0, 0, 8, 0, 1 << 12)
        times = []
        for _ in range(reps):
            got, dt = timed_grind(ctx, state, 60, 0, units)
            assert got is None
            times.append(dt)
        grind_s = sorted(times)[len(times) // 2]
        # the permutation over the same number of units, resident on the device
        n = min(units, 1 << 22)
        host = synth.random_elements(cfg.field, n * cfg.t, seed=7).reshape(n, cfg.t, 4)
        d = torch.from_numpy(host.view(np.int64)).cuda()
        launches = units // n
        ctx.permute_batch_dev(d.data_ptr(), n)
        torch.cuda.synchronize()
        ptimes = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                ctx.permute_batch_dev(d.data_ptr(), n)
            b.record()
            torch.cuda.synchronize()
            ptimes.append(a.elapsed_time(b) * 1e-3)
        perm_s = sorted(ptimes)[len(ptimes) // 2]
        print(json.dumps({"what": "long", "config": label, "units": units, "grind_ms": round(1e3 * grind_s, 3),
                          "grind_candidates_per_s": round(units / grind_s), "permute_units_per_launch": n, "permute_launches": launches,
                          "permute_ms": round(1e3 * perm_s, 3), "permutations_per_s": round(units / perm_s),
                          "grind_over_permute": round((units / grind_s) / (units / perm_s), 4),
                          "grind_engine": engine(ctx, _lib.OP_GRIND, 1 << 20),
                          "permute_engine": engine(ctx, _lib.OP_PERMUTE, n)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["sweep", "long"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--units-log2", type=int, default=26)
    a = ap.parse_args()
    if "sweep" in a.what:
        _lib.use_test_library()
        sweep(a.reps)
    if "long" in a.what:
        long_search(a.reps, a.units_log2)
