#!/usr/bin/env python3
"""Times of the matrix commitment (pmx_matrix_commit) on the device, for profiles/matrix_commit/README.md.  Everything runs on the test
library (the shipped objects plus the hooks), on page-locked host memory, t = 3 BLS12-381 Fr and t = 9 BN254 Fr, n_rows = 2^20,
row_len 8 and 64 unless told otherwise; medians of `reps` calls after one warm-up call.

  call     pmx_matrix_commit on the column-major matrix (nodes and root back) against what a caller had to do before it existed: a numpy
           transpose into a row-major buffer, pmx_hash_batch(out_len = 1), pmx_merkle_ragged over the leaves - each piece and the sum -
           and, alongside, the time the link alone takes for the matrix bytes (pmx_device_upload).  The two node arrays must be equal.
  kernel   the strided hash kernel on a device-resident column-major matrix (pmx_test_matrix_leaves_dev, strides (1, n_rows)) against
           pmx_hash_batch_dev on the row-major copy, events around single launches, the two alternating; the spread of
           pmx_hash_batch_dev over the session is reported with it.  The digests must be equal.
  slabs    whole-call time of pmx_matrix_commit against the slab size, powers of two from 1 MiB up to the matrix, set through
           pmx_test_matrix_slab_rows - every size runs the product's own host loop.
  clock    the shader clock of the box under a dense multiply stream (the benchmark diagnostics), noted once.
usage: matrix_commit_rate.py [clock] [call] [kernel] [slabs] [--reps R] [--rows-log2 L] [--row-lens 8,64]      one JSON line per measurement"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import sponge_amd as S  # noqa: E402
from sponge_amd import _lib  # noqa: E402
from sponge_amd.poseidon import merkle_ragged_shape  # noqa: E402

CONFIGS = {"t3-bls": (S.BLS12_381_FR, 2, 5, 8, 31), "t9-bn254": (S.BN254_FR, 8, 5, 8, 57)}
COL = _lib.MATRIX_COL_MAJOR
ARITY = 2


def median(xs):
    return sorted(xs)[len(xs) // 2]


def ms(x):
    return round(1e3 * x, 3)


class Pinned:
    """a page-locked block (pmx_host_alloc) seen as a numpy array"""

    def __init__(self, shape, dtype=np.uint64):
        self.ptr = ctypes.c_void_p()
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        _lib.check(_lib.lib().pmx_host_alloc(ctypes.byref(self.ptr), nbytes))
        self.array = np.frombuffer((ctypes.c_char * nbytes).from_address(self.ptr.value), dtype=dtype).reshape(shape)

    def free(self):
        self.array = None
        _lib.check(_lib.lib().pmx_host_free(self.ptr))


def fill_reduced(a, seed):
    """fully reduced residues without a field multiplication per element: random limbs, the top one below 2^60 (both moduli exceed 2^253)"""
    rng = np.random.default_rng(seed)
    flat = a.reshape(-1, 4)
    step = 1 << 22
    for i in range(0, flat.shape[0], step):
        part = rng.integers(0, 1 << 63, (min(step, flat.shape[0] - i), 4), dtype=np.uint64)
        part[:, 3] >>= np.uint64(3)
        flat[i:i + step] = part


def setup(label):
    f, rate, alpha, rf, rp = CONFIGS[label]
    cfg = S.poseidon_config_from_lfsr(f, rate, alpha, rf, rp)
    return cfg, cfg.context(0)


def engine(ctx, n, row_len):
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(ctx._h, _lib.OP_HASH, n, row_len, ctypes.byref(info)))
    return info.engine.decode()


def timed(fn, reps):
    fn()                                                       # warm-up: module load, staging buffers
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return times


def commit_into(ctx, matrix, n_rows, row_len, nodes, root):
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    _lib.check(_lib.lib().pmx_matrix_commit(ctx._h, p(matrix), n_rows, row_len, COL, ARITY, p(nodes), p(root)))


def call(label, n_rows, row_len, reps):
    cfg, ctx = setup(label)
    lib = _lib.lib()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    _, n_nodes = merkle_ragged_shape(n_rows, ARITY)
    col, row, leaves = Pinned((row_len, n_rows, 4)), Pinned((n_rows, row_len, 4)), Pinned((n_rows, 4))
    nodes, old_nodes, root = Pinned((n_nodes, 4)), Pinned((n_nodes, 4)), Pinned((4,))
    try:
        fill_reduced(col.array, seed=row_len)
        new = timed(lambda: commit_into(ctx, col.array, n_rows, row_len, nodes.array, root.array), reps)

        def transpose():
            np.copyto(row.array, col.array.transpose(1, 0, 2))

        def hash_rows():
            _lib.check(lib.pmx_hash_batch(ctx._h, p(row.array), row_len, p(leaves.array), 1, n_rows))

        def tree():
            _lib.check(lib.pmx_merkle_ragged(ctx._h, p(leaves.array), n_rows, ARITY, p(old_nodes.array), p(root.array)))

        def old_path():
            transpose()
            hash_rows()
            tree()
        old = timed(old_path, reps)
        pieces = {name: ms(median(timed(fn, reps))) for name, fn in (("transpose", transpose), ("hash_batch", hash_rows), ("merkle_ragged", tree))}
        assert nodes.array.tobytes() == old_nodes.array.tobytes(), "the two paths disagree"
        # the link alone: the matrix bytes from page-locked memory into device memory
        d = ctypes.c_void_p()
        _lib.check(lib.pmx_device_alloc(0, ctypes.byref(d), col.array.nbytes))

        def link():
            _lib.check(lib.pmx_device_upload(0, d, p(col.array), col.array.nbytes, None))
            _lib.check(lib.pmx_stream_synchronize(0, None))
        link_s = median(timed(link, reps))
        _lib.check(lib.pmx_device_free(0, d))
        print(json.dumps({"what": "call", "config": label, "n_rows": n_rows, "row_len": row_len, "matrix_mib": col.array.nbytes >> 20,
                          "commit_ms_median": ms(median(new)), "commit_ms_min": ms(min(new)), "commit_ms_max": ms(max(new)),
                          "old_path_ms_median": ms(median(old)), "old_path_ms_min": ms(min(old)), "old_path_ms_max": ms(max(old)),
                          "old_over_new": round(median(old) / median(new), 3), "old_pieces_ms_median": pieces, "link_only_ms_median": ms(link_s),
                          "link_gb_per_s": round(col.array.nbytes / link_s / 1e9, 1), "engine": engine(ctx, n_rows, row_len), "reps": reps}), flush=True)
    finally:
        for b in (col, row, leaves, nodes, old_nodes, root):
            b.free()


def kernel(label, n_rows, row_len, reps):
    import torch
    cfg, ctx = setup(label)
    lib = _lib.lib()
    host = np.empty((row_len, n_rows, 4), dtype=np.uint64)
    fill_reduced(host, seed=100 + row_len)
    d_col = torch.from_numpy(host.view(np.int64)).cuda()
    d_row = d_col.permute(1, 0, 2).contiguous()
    d_a, d_b = torch.zeros((n_rows, 4), dtype=torch.int64, device="cuda"), torch.zeros((n_rows, 4), dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def strided():
        _lib.check(lib.pmx_test_matrix_leaves_dev(ctx._h, d_col.data_ptr(), n_rows, row_len, 1, n_rows, d_a.data_ptr(), st))

    def row_major():
        _lib.check(lib.pmx_hash_batch_dev(ctx._h, d_row.data_ptr(), row_len, d_b.data_ptr(), 1, n_rows, st))
    times = {"strided": [], "row_major": []}
    for fn in (strided, row_major):
        fn()
    torch.cuda.synchronize()
    assert torch.equal(d_a, d_b), "the two kernels disagree"
    for _ in range(reps):
        for name, fn in (("strided", strided), ("row_major", row_major)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) * 1e-3)
    s, r = times["strided"], times["row_major"]
    print(json.dumps({"what": "kernel", "config": label, "n_rows": n_rows, "row_len": row_len,
                      "col_major_strided_ms": {"median": ms(median(s)), "min": ms(min(s)), "max": ms(max(s))},
                      "row_major_hash_batch_dev_ms": {"median": ms(median(r)), "min": ms(min(r)), "max": ms(max(r))},
                      "row_major_spread": round((max(r) - min(r)) / median(r), 4), "strided_over_row_major": round(median(s) / median(r), 4),
                      "engine": engine(ctx, n_rows, row_len), "reps": reps}), flush=True)


def slabs(label, n_rows, row_len, reps):
    cfg, ctx = setup(label)
    lib = _lib.lib()
    _, n_nodes = merkle_ragged_shape(n_rows, ARITY)
    col, nodes, root = Pinned((row_len, n_rows, 4)), Pinned((n_nodes, 4)), Pinned((4,))
    try:
        fill_reduced(col.array, seed=row_len)
        want = None
        log2 = 20
        while True:
            rows = max(1, (1 << log2) // (32 * row_len))
            _lib.check(lib.pmx_test_matrix_slab_rows(rows))
            times = timed(lambda: commit_into(ctx, col.array, n_rows, row_len, nodes.array, root.array), reps)
            want = want or nodes.array.tobytes()
            assert nodes.array.tobytes() == want, ("the result depends on the slab size", log2)
            print(json.dumps({"what": "slabs", "config": label, "n_rows": n_rows, "row_len": row_len, "slab_bytes_log2": log2, "slab_rows": min(rows, n_rows),
                              "slabs": -(-n_rows // rows), "ms_median": ms(median(times)), "ms_min": ms(min(times)), "ms_max": ms(max(times)), "reps": reps}),
                  flush=True)
            if rows >= n_rows:
                break
            log2 += 1
    finally:
        _lib.check(lib.pmx_test_matrix_slab_rows(0))
        for b in (col, nodes, root):
            b.free()


def clock():
    peak = _lib.PmxValuPeak()
    _lib.check_diag(_lib.diag_lib().pmx_diag_int_valu_peak(0, 0.1, ctypes.byref(peak)))
    print(json.dumps({"what": "clock", "shader_clock_mhz": round(peak.shader_clock_hz / 1e6, 1), "compute_units": peak.compute_units}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["clock", "call", "kernel", "slabs"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows-log2", type=int, default=20)
    ap.add_argument("--row-lens", default="8,64")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    a = ap.parse_args()
    _lib.use_test_library()
    if "kernel" in a.what:
        import torch
        torch.cuda.init()                                      # torch's HIP runtime first, as in the tests
    if "clock" in a.what:
        clock()
    for what, fn in (("call", call), ("kernel", kernel), ("slabs", slabs)):
        if what in a.what:
            for label in a.configs.split(","):
                for row_len in (int(x) for x in a.row_lens.split(",")):
                    fn(label, 1 << a.rows_log2, row_len, a.reps)
