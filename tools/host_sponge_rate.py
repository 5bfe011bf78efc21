#!/usr/bin/env python3
"""Wall time of the host-buffer sponge entries on pageable buffers (pmx_sponge.cpp: sponge_host, squeeze_cut_host, varlen_host), per
step, BLS12-381 Fr t = 3 (rate 2):
  packed n=1            one sponge, absorb(3) + squeeze(3): the page-locked block of a small call, one copy each way
  absorb(8) / squeeze(3) / squeeze_bytes(32) / absorb_varlen(0..8)     2^16 sponges: the resident walk with one piece
  --long                once each, not a row of samples: absorb(65536 rates + 1) and squeeze(65536 rates + one rate) on 3 sponges, the
                        walk with two pieces (tests/test_gpu_sponge_passes.py has the same calls against the C oracle)
Every row is the median, minimum and maximum of --steps calls after a warm-up; --library PATH binds another build (the parent's) so
that two builds are timed by the same script.  Prints one JSON line.
usage: python tools/host_sponge_rate.py [--steps 20] [--library PATH] [--long]"""
import argparse
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
ap.add_argument("--long", action="store_true")
ARGS = ap.parse_args()
if ARGS.library:
    _lib.use_library(os.path.abspath(ARGS.library), older_build=True)

import sponge_amd as S  # noqa: E402
from sponge_amd import synth  # noqa: E402

WARMUP = 3
f = S.BLS12_381_FR
cfg = S.poseidon_config_from_lfsr(f, 2, 5, 8, 31)


def row(fn, steps):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "steps": steps}


def batch(n, seed):
    b = S.BatchPoseidonSponge.new(cfg, n)
    b.state = synth.random_elements(f, n * 3, seed=seed).reshape(n, 3, 4)
    return b


out = {"tool": "host_sponge_rate", "library": os.path.abspath(_lib.library_path()), "warmup": WARMUP, "rows": {}}
one, msg = batch(1, 1), f.from_ints([0, 1, 2]).reshape(1, 3, 4)
out["rows"]["packed n=1 absorb(3)+squeeze(3)"] = row(lambda: (one.absorb(msg), one.squeeze_native_field_elements(3)), 10 * ARGS.steps)
n = 1 << 16
many = batch(n, 2)
elems = synth.random_elements(f, n * 8, seed=3).reshape(n, 8, 4)
lengths = np.arange(n) % 9
offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
ragged = np.ascontiguousarray(elems.reshape(-1, 4)[:int(offsets[-1])])
out["rows"]["absorb(8) n=65536"] = row(lambda: many.absorb(elems), ARGS.steps)
out["rows"]["squeeze(3) n=65536"] = row(lambda: many.squeeze_native_field_elements(3), ARGS.steps)
out["rows"]["squeeze_bytes(32) n=65536"] = row(lambda: many.squeeze_bytes(32), ARGS.steps)
out["rows"]["absorb_varlen(0..8) n=65536"] = row(lambda: many.absorb_varlen(ragged, offsets), ARGS.steps)
if ARGS.long:
    few = batch(3, 4)
    few.mode_tag, few.mode_index = np.array([0, 1, 1], dtype=np.uint32), np.array([1, 1, 2], dtype=np.uint32)
    long_in = synth.random_elements(f, 3 * (65536 * 2 + 1), seed=5).reshape(3, 65536 * 2 + 1, 4)
    t0 = time.perf_counter()
    few.absorb(long_in)
    t1 = time.perf_counter()
    few.squeeze_native_field_elements(1)        # every sponge inside its rate
    t2 = time.perf_counter()
    few.squeeze_native_field_elements(65536 * 2 + 2)
    t3 = time.perf_counter()
    out["long n=3"] = {"absorb(131073)_ms": round((t1 - t0) * 1e3, 1), "squeeze(131074)_ms": round((t3 - t2) * 1e3, 1)}
print(json.dumps(out))
