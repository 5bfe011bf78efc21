"""What sponge_amd/csrc/Makefile rebuilds when a header changes - no GPU, nothing compiled.

The objects' dependencies are the compiler's (-MMD, build/*.d), so a host header rebuilds host objects only and a device header only the
device translation units that include it.  On the tree as build() left it, `make -n -W <header>` pretends the header is new and prints what
it would run; the object names are read off the `-o build/<name>.o` of those lines and compared with the sets stated here."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sponge_amd", "csrc")

WINDOW = {"pmx_device_window_%d" % n for n in range(1, 9)}
DEVICE = WINDOW | {"pmx_device", "pmx_tree_moves", "pmx_convert", "pmx_diag"}
API = {"pmx_context", "pmx_host_call", "pmx_batch", "pmx_sponge", "pmx_matrix"}
HOST = API | {"pmx_merkle", "pmx_mgpu", "pmx_mgpu_test", "pmx_hooks", "pmx_hooks_test", "pmx_params"}

# header -> (objects that must be rebuilt, objects that must not be)
CASES = {
    "pmx_ctx.hpp": (API, DEVICE),
    "pmx_staging.hpp": (API, DEVICE),
    "pmx_prepare.hpp": ({"pmx_context"}, DEVICE | {"pmx_batch", "pmx_sponge", "pmx_matrix", "pmx_merkle"}),
    "pmx_matrix_shape.hpp": ({"pmx_matrix"}, {"pmx_sponge", "pmx_batch", "pmx_context"}),
    "pmx_grind_plan.hpp": ({"pmx_sponge"}, {"pmx_matrix", "pmx_batch", "pmx_context"}),
    "pmx_field.hpp": (WINDOW | {"pmx_device", "pmx_convert"}, set()),
    "pmx_engines.hpp": (WINDOW | {"pmx_device"}, HOST | {"pmx_tree_moves"}),
}


def make(*args):
    return subprocess.run(["make", "-C", CSRC, *args, "all"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def rebuilt(header):
    r = make("-n", "-W", header)
    assert r.returncode == 0, r.stdout
    return set(re.findall(r"-o build/(\w+)\.o\b", r.stdout))


def test_the_object_sets_are_the_makefiles():
    """every object `make -n -B` would compile is in one of the two sets above, and the other way round"""
    r = make("-n", "-B")
    assert r.returncode == 0, r.stdout
    assert set(re.findall(r"-c \S+ -o build/(\w+)\.o\b", r.stdout)) == DEVICE | HOST


def test_a_built_tree_is_up_to_date():
    r = make("-q")
    assert r.returncode == 0, "make -q says sponge_amd/csrc is not up to date (was it built?):\n" + r.stdout


@pytest.mark.parametrize("header", sorted(CASES))
def test_a_header_rebuilds_the_objects_that_include_it(header):
    assert os.path.exists(os.path.join(CSRC, header))
    must, must_not = CASES[header]
    got = rebuilt(header)
    assert got <= DEVICE | HOST, got
    assert must <= got, sorted(must - got)
    assert not (must_not & got), sorted(must_not & got)
