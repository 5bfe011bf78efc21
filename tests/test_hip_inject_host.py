"""The detector of tests/test_gpu_hip_failures.py, checked without a device: pmx::hip_inject of sponge_amd/csrc/pmx_hooks.cpp, the one
function every checked HIP call of the single-device entries asks first, compiled into tests/hip_inject/hip_inject_host.cpp - a program
of its own under ASan + UBSan (host side only; the file needs the HIP headers, so the compiler is hipcc).
- built -DPMX_TEST_HOOKS, as for libposeidon_mi355x_test.so: the count, arming, the one shot, the call that is NOT made, the wording, and
  thread-locality - a second std::thread is neither counted nor failed;
- built without, as for the library that ships: hipSuccess, always, and nothing to ask about."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sponge_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "hip_inject", "hip_inject_host.cpp")


def hipcc():
    found = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"     # (the Makefile's default)
    assert os.path.exists(found), "the build needs hipcc, and so does this test"
    return found


@pytest.mark.parametrize("variant,define", [("test", ["-DPMX_TEST_HOOKS"]), ("shipped", [])])
def test_the_injector_under_asan_and_ubsan(tmp_path, variant, define):
    exe = str(tmp_path / f"hip_inject_{variant}")
    subprocess.check_call([hipcc(), "-O1", "-g", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Wno-unused-parameter", *define, "-I", CSRC, SRC,
                           "-fsanitize=address,undefined", "-pthread", "-o", exe], cwd=str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{variant} variant ok" in out.stdout
