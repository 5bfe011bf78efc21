"""bench.py --dump-outputs on the GPU: two runs whose spin-ups take different numbers of steps write the same arrays, and those
arrays are what the timed path computed - the seeded batch after W + K permutations (the spin-up's state does not carry over),
and the digests of the hash driver - checked against the C restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sponge_amd as S
from sponge_amd import synth

from gpu_helpers import c_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd + list(extra), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    return {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}


def limbs(a):
    return a.astype(np.uint8).view(np.uint64)


def test_dump_outputs_of_the_permutation_batch_are_its_last_step(tmp_path):
    n = 1 << 12
    a = run_bench(tmp_path / "a", "--total-log2", "12", "--spinup-seconds", "0.05")
    b = run_bench(tmp_path / "b", "--total-log2", "12", "--spinup-seconds", "0.3")
    assert sorted(a) == ["states"] and a["states"].dtype == np.float32 and np.array_equal(a["states"], b["states"])
    x = synth.random_elements(S.BLS12_381_FR, n * 3, 0x5EED0002).reshape(n, 3, 4)
    cr = c_oracle("bls_t3_a5_8_31")
    for _ in range(3):                                    # W + K = 1 + 2 steps, each permuting in place
        x = cr.permute_batch(x, threads=0)
    assert np.array_equal(limbs(a["states"]), x)


def test_dump_outputs_of_the_hash_driver_sample_the_rows(tmp_path):
    n = 1 << 16                                           # more rows than a dump keeps: a seeded sample of them
    a = run_bench(tmp_path / "a", "--workload", "h3", "--total-log2", "16", "--spinup-seconds", "0.05")
    b = run_bench(tmp_path / "b", "--workload", "h3", "--total-log2", "16", "--spinup-seconds", "0.3")
    assert sorted(a) == ["digests", "digests_rows"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = a["digests_rows"].astype(np.int64)
    msgs = synth.random_elements(S.BLS12_381_FR, n * 4, 0x5EED0006).reshape(n, 4, 4)[rows]
    want = c_oracle("bls_t3_a5_8_31").hash_batch(np.ascontiguousarray(msgs), 4, 1, threads=0)
    assert np.array_equal(limbs(a["digests"]).reshape(len(rows), 1, 4), want.reshape(len(rows), 1, 4))
