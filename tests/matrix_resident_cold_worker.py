"""Child process of tests/test_gpu_matrix_resident.py::test_cold_chain_capture_in_a_fresh_process: the commit, open and verify chain of
include/poseidon_mi355x_resident.h captured into ONE graph with nothing warmed up.

A fresh process creates a context and captures pmx_matrix_commit_dev, pmx_matrix_open_dev and pmx_matrix_verify_rows_dev, one behind the
other on one stream, as the first launches of any kernel of the library in the process: the opening reads the node array the commit
writes, the verifier reads the opened rows, their paths and the root where the commit leaves it.  Capturing must execute nothing; the
replay must give the values the parent computed with the oracle and left as .npy files in the directory given as the only argument.
Nothing here reads the oracle.  Exit status 0 and a last line "cold chain ok" on success."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sponge_amd as S                    # noqa: E402
from sponge_amd import _lib               # noqa: E402


def main(directory):
    load = lambda name: np.load(os.path.join(directory, name + ".npy"))
    matrix, indices, nodes, rows, paths, ok = (load(name) for name in ("matrix", "indices", "nodes", "rows", "paths", "ok"))
    n_rows, row_len, row_stride, elem_stride, arity, k = (int(x) for x in load("shape"))
    depth = paths.shape[1]
    cfg = S.poseidon_config_from_lfsr(S.BLS12_381_FR, 2, 5, 8, 31)
    ctx = cfg.context()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to("cuda:0")
    fill = lambda nbytes, byte: torch.full((nbytes,), byte, dtype=torch.uint8, device="cuda:0")
    d_matrix, d_idx = up(matrix), up(indices)
    d_nodes, d_rows, d_paths = fill(nodes.nbytes, 0xA5), fill(rows.nbytes, 0xA6), fill(paths.nbytes, 0xA7)
    d_ok, d_work = fill(k, 0xA8), fill(k * (arity + 2) * 32, 0xA9)
    outputs = (d_nodes, d_rows, d_paths, d_ok, d_work)
    before = [t.clone() for t in outputs]
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(device="cuda:0"), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="global"):
        st = torch.cuda.current_stream().cuda_stream
        ctx.matrix_commit_dev(d_matrix.data_ptr(), n_rows, row_len, row_stride, elem_stride, arity, d_nodes.data_ptr(), st)
        ctx.matrix_open_dev(d_matrix.data_ptr(), n_rows, row_len, row_stride, elem_stride, d_nodes.data_ptr(), arity, d_idx.data_ptr(), k,
                            d_rows.data_ptr(), d_paths.data_ptr(), st)
        ctx.matrix_verify_rows_dev(d_rows.data_ptr(), row_len, d_idx.data_ptr(), d_paths.data_ptr(), depth, arity, n_rows, k,
                                   d_nodes.data_ptr() + (nodes.shape[0] - 1) * 32, d_ok.data_ptr(), d_work.data_ptr(), st)
    torch.cuda.synchronize()
    assert all(torch.equal(b, t) for b, t in zip(before, outputs)), "capturing changed a buffer"
    g.replay()
    torch.cuda.synchronize()
    for what, t, want in (("nodes", d_nodes, nodes), ("rows", d_rows, rows), ("paths", d_paths, paths), ("ok", d_ok, ok)):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes(), f"{what}: the replay differs from the expected values"
        print(f"{what}: captured cold, replayed, bit-exact")
    assert _lib.lib().pmx_abi_version() == _lib.ABI_VERSION
    print("cold chain ok")


if __name__ == "__main__":
    main(sys.argv[1])
