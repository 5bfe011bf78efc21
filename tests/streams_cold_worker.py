"""Child process of tests/test_gpu_streams.py::test_cold_capture_in_a_fresh_process: graph capture with nothing warmed up.

A fresh process creates a context and captures pmx_permute_batch_dev into a graph as the first launch of any kernel of the library in
the process, then does the same with a 512-leaf pmx_merkle_2to1_dev (the first launch of the compression kernel).  Capturing must
execute nothing; the replay must give the values the parent computed with the oracle and left as .npy files in the directory given as
the only argument.  Nothing here reads the oracle.  Exit status 0 and a last line "cold capture ok" on success."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sponge_amd as S                    # noqa: E402
from sponge_amd import _lib               # noqa: E402


def captured(what, call, dev, want):
    before = dev.clone()
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(device="cuda:0"), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="global"):
        rc = call(torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.PMX_OK, (what, rc, _lib.lib().pmx_last_error())
    torch.cuda.synchronize()
    assert torch.equal(before, dev), f"{what}: capturing changed the buffer"
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy().view(np.uint64).reshape(want.shape), want), f"{what}: the replay differs from the expected values"
    print(f"{what}: captured cold, replayed, bit-exact")


def main(directory):
    states, permuted, first, nodes = (np.load(os.path.join(directory, name + ".npy")) for name in ("states", "permuted", "first", "nodes"))
    cfg = S.poseidon_config_from_lfsr(S.BLS12_381_FR, 2, 5, 8, 31)
    h, L = cfg.context()._h, _lib.lib()
    dev = torch.from_numpy(states.reshape(-1).view(np.uint8)).to("cuda:0")
    captured("pmx_permute_batch_dev", lambda st: L.pmx_permute_batch_dev(h, dev.data_ptr(), states.shape[0], st), dev, permuted)
    tree = torch.from_numpy(first.reshape(-1).view(np.uint8)).to("cuda:0")
    captured("pmx_merkle_2to1_dev", lambda st: L.pmx_merkle_2to1_dev(h, tree.data_ptr(), (first.shape[0] + 1) // 2, st), tree, nodes)
    print("cold capture ok")


if __name__ == "__main__":
    main(sys.argv[1])
