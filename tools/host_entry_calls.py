#!/usr/bin/env python3
"""Which HIP runtime calls every host-buffer entry makes, for comparing two builds of the library (profiles/host_call_scope/README.md).

  python tools/host_entry_calls.py [--library PATH]       drive: every host-buffer entry once at its smallest shape and once at a shape
        that grows its staging blocks, and - where an entry walks in pieces and the test library has a hook for the piece size - one
        call of several pieces.  No result is checked (tests/test_gpu_host_staging.py does that).  In front of every call the driver
        makes one hipHostMalloc / hipHostFree pair through pmx_host_alloc / pmx_host_free: no entry frees page-locked memory, so the
        pair cuts the trace into calls.  Run it under the HIP API tracer, the interpreter behind `--`:
            rocprofv3 --hip-runtime-trace --output-format csv -d OUT -- python tools/host_entry_calls.py [--library PATH]
        --library: the test-hook build (libposeidon_mi355x_test.so) of another commit; default: this tree's.
  python tools/host_entry_calls.py --names TRACE.csv      the ordered HIP API names per call, one line per call, from the tracer's
        *_hip_api_trace.csv
  python tools/host_entry_calls.py --compare A.txt B.txt [--labels LABELS]   the calls whose lists differ, with the counts per API name"""
import argparse
import collections
import csv
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--library", default=None)
ap.add_argument("--names", default=None)
ap.add_argument("--compare", nargs=2, default=None)
ap.add_argument("--labels", default=None, help="the names of the calls, one a line: written by the drive (default host_entry_calls_labels.txt), read by --compare")
ARGS = ap.parse_args()

CALLS = []      # the labels, in the order of the calls


def names(path):
    """the HIP API names of every call: the trace in start order, cut at the marker pairs (a hipHostMalloc in front of a hipHostFree)"""
    with open(path, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur, last = [], None, None
    for r in rows:
        fn = r["Function"]
        if fn == "hipHostFree" and last == "hipHostMalloc":     # (a context that is destroyed frees its page-locked block: no marker)
            if cur:
                cur.pop()
            cur = []
            calls.append(cur)
        elif cur is not None:
            cur.append(fn)
        last = fn
    return calls


if ARGS.names:
    for i, c in enumerate(names(ARGS.names)):
        print(i, " ".join(c))
    sys.exit(0)

if ARGS.compare:
    a, b = ([line.split()[1:] for line in open(p)] for p in ARGS.compare)
    labels = [line.strip() for line in open(ARGS.labels)] if ARGS.labels else []
    print(f"{len(a)} calls against {len(b)}")
    differ = 0
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            differ += 1
            cx, cy = collections.Counter(x), collections.Counter(y)
            delta = {k: cy[k] - cx[k] for k in sorted(set(cx) | set(cy)) if cx[k] != cy[k]}
            print(f"call {i} {labels[i] if i < len(labels) else ''}: {len(x)} -> {len(y)} API calls; counts that differ (B - A): {delta}"
                  + ("" if delta else "; same counts, another order"))
    print(f"{differ} calls differ")
    sys.exit(0)

from sponge_amd import _lib  # noqa: E402

if ARGS.library:
    _lib.use_library(os.path.abspath(ARGS.library), test_hooks=True, older_build=True)
else:
    _lib.use_test_library()

import numpy as np  # noqa: E402
import sponge_amd as S  # noqa: E402
from sponge_amd import synth  # noqa: E402
from sponge_amd.poseidon import Context, c_config, merkle_ragged_shape  # noqa: E402

L = _lib.lib()


def call(label, fn):
    p = ctypes.c_void_p()
    _lib.check(L.pmx_host_alloc(ctypes.byref(p), 16))
    _lib.check(L.pmx_host_free(p))
    CALLS.append(label)
    fn()


def drive(f, rate, rp, arity):
    cfg = S.poseidon_config_from_lfsr(f, rate, 5, 8, rp)
    c, handle = c_config(cfg), ctypes.c_void_p()
    _lib.check(L.pmx_ctx_create(ctypes.byref(c), 0, ctypes.byref(handle)))
    ctx, t, who = Context.borrowed(cfg, 0, handle.value), cfg.t, f"t={cfg.t}"
    rng = np.random.default_rng(1)

    def sponges(n):
        return (synth.random_elements(f, n * t, seed=n).reshape(n, t, 4), rng.integers(0, 2, n).astype(np.uint32),
                rng.integers(0, rate + 1, n).astype(np.uint32))

    for big in (False, True):
        tag = f"{who} {'grown' if big else 'small'}"
        n = 400 if big else 1
        call(f"{tag} permute_batch", lambda: ctx.permute_batch(synth.random_elements(f, n * t, seed=2).reshape(n, t, 4)))
        call(f"{tag} hash_batch", lambda: ctx.hash_batch(synth.random_elements(f, n * 5, seed=3).reshape(n, 5, 4), 5, 2))
        st = sponges(n)
        call(f"{tag} sponge_absorb_batch", lambda: ctx.sponge_absorb_batch(*st, synth.random_elements(f, n * 3, seed=4).reshape(n, 3, 4), 3))
        call(f"{tag} sponge_squeeze_batch", lambda: ctx.sponge_squeeze_batch(*st, 3))
        call(f"{tag} sponge_squeeze_bytes_batch", lambda: ctx.sponge_squeeze_bytes_batch(*st, 70))
        call(f"{tag} sponge_squeeze_bits_batch", lambda: ctx.sponge_squeeze_bits_batch(*st, 300))
        call(f"{tag} sponge_grind", lambda: ctx.sponge_grind(st[0][0], int(st[1][0]), int(st[2][0]), 3, 0, 64))
        lengths = rng.integers(0, 8, n) if big else np.array([2])
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
        elems = synth.random_elements(f, int(offsets[-1]), seed=5)
        call(f"{tag} sponge_absorb_varlen_batch", lambda: ctx.sponge_absorb_varlen_batch(*st, elems, offsets))
        call(f"{tag} hash_varlen_batch", lambda: ctx.hash_varlen_batch(elems, offsets, 2))
        n_rows, row_len = (600, 7) if big else (5, 3)
        m = synth.random_elements(f, n_rows * row_len, seed=6)
        for layout in (_lib.MATRIX_ROW_MAJOR, _lib.MATRIX_COL_MAJOR):
            call(f"{tag} matrix_leaves layout {layout}", lambda: ctx.matrix_leaves(m, n_rows, row_len, layout))
            call(f"{tag} matrix_commit layout {layout}", lambda: ctx.matrix_commit(m, n_rows, row_len, layout, arity))
        depth, n_nodes = merkle_ragged_shape(n_rows, arity)
        k = 200 if big else 1
        idx = rng.integers(0, n_rows, k).astype(np.uint64)
        paths = synth.random_elements(f, k * depth * (arity - 1), seed=7).reshape(k, depth, arity - 1, 4)
        root = synth.random_elements(f, 1, seed=8)[0]
        call(f"{tag} matrix_verify_rows", lambda: ctx.matrix_verify_rows(m.reshape(n_rows, row_len, 4)[:k].copy(), idx, paths, depth, arity, n_rows, root))
        call(f"{tag} merkle_ragged_verify_paths", lambda: ctx.merkle_ragged_verify_paths(m[:k].copy(), idx, paths, depth, arity, n_rows, root))
        d = 5 if big else 1
        leaves = synth.random_elements(f, arity ** d, seed=9)
        call(f"{tag} merkle_ary", lambda: ctx.merkle_ary(leaves, arity))
        call(f"{tag} merkle_ary_forest", lambda: ctx.merkle_ary_forest(leaves, arity, arity) if big else ctx.merkle_ary_forest(leaves, 1, arity))
        if arity == 2:
            call(f"{tag} merkle_2to1", lambda: ctx.merkle_2to1(leaves))
            call(f"{tag} merkle_2to1_forest", lambda: ctx.merkle_2to1_forest(leaves, 2 if big else 1))
        call(f"{tag} merkle_ragged", lambda: ctx.merkle_ragged(m[:777 if big else 1], arity))
        ki = np.arange(k, dtype=np.uint64) % np.uint64(arity ** d)
        kp = synth.random_elements(f, k * d * (arity - 1), seed=10).reshape(k, d, arity - 1, 4)
        call(f"{tag} merkle_ary_verify_paths", lambda: ctx.merkle_ary_verify_paths(m[:k].copy(), ki, kp, d, arity, root))
        nodes = None

        def build():
            nonlocal nodes
            nodes = ctx.merkle_ary(leaves, arity)[0]
        call(f"{tag} merkle_ary again, for its node array", build)
        call(f"{tag} merkle_ary_update", lambda: ctx.merkle_ary_update(nodes, arity ** d, arity, ki[:40], m[:min(k, 40)]))
        fd, fn_ = (8, 150) if big else (1, 1)     # (the grown depth is the one of the walks in pieces below)
        e = None

        def defaults():
            nonlocal e
            e = ctx.merkle_fixed_defaults(root, arity, fd)
        call(f"{tag} merkle_fixed_defaults", defaults)
        call(f"{tag} merkle_fixed", lambda: ctx.merkle_fixed(m[:fn_], arity, fd, e))
        call(f"{tag} merkle_frontier_append", lambda: ctx.merkle_frontier_append(arity, fd, e, None, 0, m[:fn_]))
    # calls of several pieces, through the test library's hooks
    who = f"{who} pieces"
    _lib.check(L.pmx_test_merkle_fixed_piece(64))
    call(f"{who} merkle_fixed_defaults, for the walks", defaults)
    call(f"{who} merkle_fixed 150 leaves in pieces of 64", lambda: ctx.merkle_fixed(m[:150], arity, 8, e))
    call(f"{who} merkle_frontier_append 150 leaves in pieces of 64", lambda: ctx.merkle_frontier_append(arity, 8, e, None, 0, m[:150]))
    _lib.check(L.pmx_test_merkle_fixed_piece(0))
    _lib.check(L.pmx_test_matrix_slab_rows(100))
    call(f"{who} matrix_commit 600 rows in slabs of 100", lambda: ctx.matrix_commit(m[:600 * 7], 600, 7, _lib.MATRIX_COL_MAJOR, arity))
    _lib.check(L.pmx_test_matrix_slab_rows(0))
    _lib.check(L.pmx_test_grind_chunk(16))
    call(f"{who} sponge_grind 64 candidates in chunks of 16", lambda: ctx.sponge_grind(st[0][0], 0, 0, 30, 0, 64))
    _lib.check(L.pmx_test_grind_chunk(0))
    call(f"{who} end", lambda: None)
    _lib.check(L.pmx_ctx_destroy(handle))


drive(S.BLS12_381_FR, 2, 31, 2)
drive(S.BN254_FR, 8, 57, 4)
with open(ARGS.labels or "host_entry_calls_labels.txt", "w") as fh:
    fh.write("\n".join(CALLS) + "\n")
print(f"{len(CALLS)} calls driven on {_lib.library_path()}")
