"""BatchPoseidonSponge::squeeze_bytes / squeeze_bits of the C++ host mirror (sponge_amd/host/poseidon_sponge.hpp): the test program
tests/cpp/test_batch_squeeze_bytes.cpp compiles against the header and the C-ABI library everywhere, and on the GPU the batch methods
must equal the single sponge's host loops (src/poseidon/mod.rs:256-286)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_batch_squeeze_bytes.cpp")
LIBDIR = os.path.join(ROOT, "sponge_amd")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp_batch_squeeze") / "test_batch_squeeze_bytes")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", SRC, "-o", out, "-L" + LIBDIR, "-lposeidon_mi355x", "-Wl,-rpath," + LIBDIR])
    return out


def test_cpp_batch_squeeze_program_builds(program):
    assert os.path.exists(program)


@pytest.mark.gpu
def test_cpp_batch_squeeze_equals_single_sponges_on_gpu(program):
    out = subprocess.run([program], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
