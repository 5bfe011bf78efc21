#!/usr/bin/env python3
"""Wall time of the host-buffer entries of a device group (pmx_mgpu.cpp) on a group of ONE device, bound to the real collective
library, pageable numpy buffers, BLS12-381 Fr t = 3 (rate 2):
  merkle_2to1 2^12 / 2^20 leaves     pmx_mgpu_merkle_2to1: upload, the tree, the root back
  permute_batch 2^16 states          pmx_mgpu_permute_batch
  hash_batch 2^16 rows               pmx_mgpu_hash_batch, rows of 4 elements, digests of 1
Every row is the median, minimum and maximum of --steps calls after a warm-up, with a checksum of what the last call returned, so that
two builds timed by this script are also seen to compute the same; --library PATH binds another build (the parent's).  Prints one JSON
line.
usage: python tools/mgpu_host_rate.py [--steps 20] [--library PATH]"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sponge_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--library", default=None)
ARGS = ap.parse_args()
if ARGS.library:
    _lib.use_library(os.path.abspath(ARGS.library), older_build=True)

import sponge_amd as S  # noqa: E402
from sponge_amd import mgpu, synth  # noqa: E402

WARMUP = 3
f = S.BLS12_381_FR
cfg = S.poseidon_config_from_lfsr(f, 2, 5, 8, 31)
lib = _lib.lib()
g = mgpu.DeviceGroup.single_process(cfg, 1)


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def row(fn, result):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(ARGS.steps):
        t0 = time.perf_counter()
        fn()                                        # (every entry returns behind its own stream synchronise)
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "steps": ARGS.steps,
            "sha256": hashlib.sha256(result().tobytes()).hexdigest()[:16]}


out = {"tool": "mgpu_host_rate", "library": os.path.abspath(_lib.library_path()), "warmup": WARMUP, "rccl": g.info()["rccl_version_str"], "rows": {}}
root = np.zeros(4, dtype=np.uint64)
for log2_n in (12, 20):
    leaves = np.ascontiguousarray(synth.random_elements(f, 1 << log2_n, seed=log2_n), dtype=np.uint64)
    out["rows"][f"merkle_2to1 2^{log2_n} leaves"] = row(lambda: _lib.check(lib.pmx_mgpu_merkle_2to1(g._h, ptr(leaves), 1 << log2_n, ptr(root))),
                                                        lambda: root)
n = 1 << 16
fresh = np.ascontiguousarray(synth.random_elements(f, n * 3, seed=5), dtype=np.uint64)
states = fresh.copy()


def permute():
    states[:] = fresh                               # (inside the timed call on both builds: the entry permutes in place)
    _lib.check(lib.pmx_mgpu_permute_batch(g._h, ptr(states), n))


out["rows"]["permute_batch 2^16 states"] = row(permute, lambda: states)
msgs = np.ascontiguousarray(synth.random_elements(f, n * 4, seed=6), dtype=np.uint64)
digests = np.zeros((n, 1, 4), dtype=np.uint64)
out["rows"]["hash_batch 2^16 rows"] = row(lambda: _lib.check(lib.pmx_mgpu_hash_batch(g._h, ptr(msgs), 4, ptr(digests), 1, n)), lambda: digests)
g.close()
print(json.dumps(out))
