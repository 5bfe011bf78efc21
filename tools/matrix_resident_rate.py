#!/usr/bin/env python3
"""pmx_matrix_commit_dev against what a caller had before (profiles/matrix_resident/README.md).  One JSON line per figure on stdout.

A column-major matrix of 2^log2 rows and `row_len` columns lives on the device (leading dimension n_rows).  Per config:
  resident  pmx_matrix_commit_dev on it - events around the call, REPS calls after one warm-up call;
  floor     on the row-major copy of the same matrix, pmx_hash_batch_dev(in_len = row_len, out_len = 1) into the head of the node array and
            pmx_merkle_ragged_dev behind it, the same way and alternating with `resident`; its own (max - min) / median is the run-to-run
            spread the comparison is read against;
  host      pmx_matrix_commit on the same column-major matrix in page-locked host memory, nodes and root back - host wall-clock;
  open      pmx_matrix_open_dev for k queries (rows and paths) on the committed tree - events.
The node arrays of the three paths are compared for equality before anything is timed.
usage: matrix_resident_rate.py [--log2 20] [--row-len 8] [--k 128] [--reps 7]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sponge_amd as S                                    # noqa: E402
from sponge_amd import _lib, synth                         # noqa: E402
from sponge_amd.poseidon import merkle_ragged_shape        # noqa: E402

CONFIGS = {"t3-bls": (S.BLS12_381_FR, 2, 5, 8, 31, 2), "t9-bn254": (S.BN254_FR, 8, 5, 8, 57, 8)}      # field, rate, alpha, RF, RP, arity


def out(**kw):
    print(json.dumps(kw), flush=True)


def summary(ms):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4),
            "runs_ms": [round(x, 4) for x in ms]}


def timed(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--row-len", type=int, default=8)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    n, L, k = 1 << args.log2, args.row_len, args.k
    peak = _lib.PmxValuPeak()
    _lib.check_diag(_lib.diag_lib().pmx_diag_int_valu_peak(0, 0.02, ctypes.byref(peak)))
    out(what="clock", shader_clock_mhz=round(peak.shader_clock_hz / 1e6, 1), compute_units=peak.compute_units, device=torch.cuda.get_device_name(0))
    lib = _lib.lib()
    for name, (f, rate, alpha, rf, rp, arity) in CONFIGS.items():
        cfg = S.poseidon_config_from_lfsr(f, rate, alpha, rf, rp)
        ctx = cfg.context(0)
        depth, n_nodes = merkle_ragged_shape(n, arity)
        tile = synth.random_elements(f, 1 << 16, seed=0x3A7).reshape(-1, 4)
        rows = np.tile(tile, (n * L // tile.shape[0], 1)).reshape(n, L, 4)
        rows[:, 0, 0] ^= np.arange(n, dtype=np.uint64) & np.uint64(0xFFFF)             # the rows differ (the low limb stays below the modulus' top)
        col = np.ascontiguousarray(rows.transpose(1, 0, 2))
        d_col, d_row = torch.from_numpy(col.reshape(-1).view(np.int64)).cuda(), torch.from_numpy(rows.reshape(-1).view(np.int64)).cuda()
        d_nodes, d_floor = torch.zeros(n_nodes * 4, dtype=torch.int64, device="cuda"), torch.zeros(n_nodes * 4, dtype=torch.int64, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def resident():
            ctx.matrix_commit_dev(d_col.data_ptr(), n, L, 1, n, arity, d_nodes.data_ptr(), st)

        def floor():
            ctx.hash_batch_dev(d_row.data_ptr(), L, d_floor.data_ptr(), 1, n, st)
            _lib.check(lib.pmx_merkle_ragged_dev(ctx._h, d_floor.data_ptr(), n, arity, st))

        # page-locked host copy of the column-major matrix, and the host entry on it
        pinned = ctypes.c_void_p()
        _lib.check(lib.pmx_host_alloc(ctypes.byref(pinned), col.nbytes))
        ctypes.memmove(pinned, col.ctypes.data, col.nbytes)
        h_nodes, h_root = np.zeros((n_nodes, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64)

        def host():
            _lib.check(lib.pmx_matrix_commit(ctx._h, pinned, n, L, _lib.MATRIX_COL_MAJOR, arity, ctypes.c_void_p(h_nodes.ctypes.data),
                                             ctypes.c_void_p(h_root.ctypes.data)))

        resident(), floor(), host()
        torch.cuda.synchronize()
        same = torch.equal(d_nodes, d_floor) and d_nodes.cpu().numpy().view(np.uint64).tobytes() == h_nodes.tobytes()
        out(what="equal", config=name, n_rows=n, row_len=L, arity=arity, node_arrays_equal=bool(same))
        res, flo, hst = [], [], []
        for _ in range(args.reps):
            res.append(timed(resident))
            flo.append(timed(floor))
        for _ in range(args.reps):
            t0 = time.perf_counter()
            host()
            hst.append((time.perf_counter() - t0) * 1e3)
        # the hash alone, strided against row-major, the same alternation
        hs, hr = [], []
        for _ in range(args.reps):
            hs.append(timed(lambda: ctx.matrix_leaves_dev(d_col.data_ptr(), n, L, 1, n, d_nodes.data_ptr(), st)))
            hr.append(timed(lambda: ctx.hash_batch_dev(d_row.data_ptr(), L, d_floor.data_ptr(), 1, n, st)))
        resident()
        idx = torch.from_numpy(np.random.default_rng(7).integers(0, n, k).astype(np.int64)).cuda()
        d_rows = torch.zeros(k * L * 4, dtype=torch.int64, device="cuda")
        d_paths = torch.zeros(max(k * depth * (arity - 1) * 4, 4), dtype=torch.int64, device="cuda")

        def opening():
            ctx.matrix_open_dev(d_col.data_ptr(), n, L, 1, n, d_nodes.data_ptr(), arity, idx.data_ptr(), k, d_rows.data_ptr(), d_paths.data_ptr(), st)

        opening()
        torch.cuda.synchronize()
        opn = [timed(opening) for _ in range(args.reps)]
        base = dict(config=name, n_rows=n, row_len=L, arity=arity)
        out(what="resident pmx_matrix_commit_dev (column-major, events)", **base, **summary(res))
        out(what="floor pmx_hash_batch_dev + pmx_merkle_ragged_dev (row-major, events)", **base, **summary(flo))
        out(what="host pmx_matrix_commit (page-locked, wall clock)", **base, **summary(hst))
        out(what="hash alone: pmx_matrix_leaves_dev (column-major)", **base, **summary(hs))
        out(what="hash alone: pmx_hash_batch_dev (row-major)", **base, **summary(hr))
        out(what="pmx_matrix_open_dev rows + paths", k=k, depth=depth, **base, **summary(opn))
        out(what="ratios", **base, resident_over_floor=round(statistics.median(res) / statistics.median(flo), 4),
            host_over_resident=round(statistics.median(hst) / statistics.median(res), 2),
            strided_over_row_major_hash=round(statistics.median(hs) / statistics.median(hr), 4))
        _lib.check(lib.pmx_host_free(pinned))
        del d_col, d_row, d_nodes, d_floor
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
