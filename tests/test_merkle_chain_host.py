"""Sequential leaf updates of a fixed-depth tree with witnesses (pmx_merkle_update_witnesses), the parts that need no device:
- tests/merkle_chain/chain_host.cpp, a program of its own under ASan + UBSan over sponge_amd/csrc/pmx_merkle_chain.hpp: the source of every
  (level, update, sibling slot), chosen from pred alone, against the overlay model walked literally - index sets with heavy collisions,
  all-equal indices, k = 1, the ends of a 2^64 tree;
- plans printed by that program against tests/merkle_chain_oracle.py's literal walk;
- the oracle's overlay model against one-at-a-time rebuilds of a dense tree (the model is what the GPU tests compare with);
- the refusals of the shipped library that fire before a context is read: each returns its status and writes nothing
  (PMX_ERR_CONFIG for arity > rate reads the context: tests/test_gpu_merkle_witness.py has it);
- the entry is declared, exported by both libraries, bound in the ctypes table and the Rust declarations, adds no *_dev entry, and the
  ABI version is still 5."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from sponge_amd import _lib, synth

import merkle_ary_oracle as MA
import merkle_chain_oracle as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sponge_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "merkle_chain", "chain_host.cpp")
ENTRY = "pmx_merkle_update_witnesses"
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def chain_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_chain") / "chain_host")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", CSRC, SRC, "-o", exe])

    def run(*args):
        out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout
    return run


def test_plan_under_asan_and_ubsan(chain_host):
    assert "sanitized ok" in chain_host()


def _index_sets(a, depth, seed):
    rng = np.random.default_rng(seed)
    cap = a ** depth
    few = min(cap, a * a + 1)
    return {
        "one": [cap - 1],
        "all equal": [cap // 3] * 7,
        "a few leaves": [int(x) for x in rng.integers(0, few, 65)],
        "the top end": [cap - 1 - int(x) for x in rng.integers(0, few, 65)],
        "ends": [0, cap - 1, cap // 2, cap // 2 - 1, 0, cap - 1],
        "anywhere": [int(rng.integers(0, 1 << 62)) % cap for _ in range(40)],
    }


@pytest.mark.parametrize("a,depth", [(2, 4), (3, 3), (8, 2), (2, 64), (8, 21), (2, 32)])
def test_printed_plans_are_the_literal_walk(chain_host, a, depth):
    for name, idx in _index_sets(a, depth, seed=10 * a + depth).items():
        lines = chain_host("plan", str(a), str(depth), *[str(i) for i in idx]).splitlines()
        got = [np.array(line.split(), dtype=np.int64).reshape(len(idx), a - 1).tolist() for line in lines]
        assert got == C.sources(a, depth, idx), (a, depth, name)


@pytest.mark.parametrize("label,a,depth", [("t3", 2, 4), ("t9-bn254", 3, 3)])
def test_the_overlay_model_is_the_tree_after_every_update(label, a, depth):
    """A test of the ORACLE, not of the product (it calls nothing of the library): with true openings in, the model's witness[j] is the
    opening in the tree rebuilt after j updates and roots[j] the root after update j; model_batched gives the model's bytes."""
    f, _, cr = MA.config(label)
    n = a ** depth
    leaves, nodes = MA.cached_tree(label, a, n)
    rng = np.random.default_rng(5)
    idx = np.array([int(x) for x in rng.integers(0, min(n, 6), 12)] + [n - 1, 0], dtype=np.uint64)
    new = synth.random_elements(f, len(idx), seed=0xC4)
    witness, roots = C.model(cr, a, depth, idx, new, MA.open_paths(nodes, n, a, idx))
    row = np.array(leaves)
    for j, i in enumerate(int(x) for x in idx):
        assert np.array_equal(witness[j], MA.open_paths(MA.tree(cr, row, a), n, a, [i])[0]), j
        row[i] = new[j]
        assert np.array_equal(roots[j], MA.tree(cr, row, a)[-1]), j
    # the level-by-level form of the model gives the same bytes, on inconsistent openings too
    for paths in (MA.open_paths(nodes, n, a, idx), synth.random_elements(f, len(idx) * depth * (a - 1), seed=3).reshape(len(idx), depth, a - 1, 4)):
        w0, r0 = C.model(cr, a, depth, idx, new, paths)
        w1, r1 = C.model_batched(cr, a, depth, idx, new, paths)
        assert np.array_equal(w0, w1) and np.array_equal(r0, r1)


# ---- the shipped library, no device ---------------------------------------------------------------------------------------------
def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_refusals_before_a_context_is_read():
    lib = _lib.lib()
    fn = lib.pmx_merkle_update_witnesses
    buf = np.zeros((64, 4), dtype=np.uint64)
    idx = np.array([3, 5], dtype=np.uint64)
    wit = np.full((2, 64, 7, 4), 0x77, dtype=np.uint64)
    roots = np.full((2, 4), 0x77, dtype=np.uint64)
    root = np.full(4, 0x77, dtype=np.uint64)
    fake = _p(buf)                                            # never dereferenced: every refusal below comes first
    i, n, p, w, r, t = _p(idx), _p(buf), _p(buf), _p(wit), _p(roots), _p(root)
    cases = [
        ((None, 2, 4, i, n, p, 2, w, r, t), b"null"),
        ((fake, 2, 4, None, n, p, 2, w, r, t), b"null"),
        ((fake, 2, 4, i, None, p, 2, w, r, t), b"null"),
        ((fake, 2, 4, i, n, None, 2, w, r, t), b"null"),
        ((fake, 1, 4, i, n, p, 2, w, r, t), b"arity"),
        ((fake, 0, 4, i, n, p, 2, w, r, t), b"arity"),
        ((fake, 2, 0, i, n, p, 2, w, r, t), b"depth"),
        ((fake, 2, 65, i, n, p, 2, w, r, t), b"depth"),
        ((fake, 3, 41, i, n, p, 2, w, r, t), b"overflows 64 bits"),
        ((fake, 8, 22, i, n, p, 2, w, r, t), b"overflows 64 bits"),
        ((fake, 2, 2, i, n, p, 2, w, r, t), b"leaf index 5 out of range"),          # 2^2 = 4 positions
        ((fake, 2, 4, i, n, p, 0, w, r, t), b"root must be NULL"),                   # k = 0: no root exists to return
        ((fake, 2, 4, None, None, None, 0, w, r, t), b"root must be NULL"),
        ((fake, 2, 4, i, n, p, (1 << 32) - 1, w, r, t), b"batch too large"),         # the documented bound: k <= 2^32 - 2
        ((fake, 2, 4, i, n, p, 1 << 40, w, r, t), b"batch too large"),
        ((fake, 2, 64, i, n, p, 1 << 63, w, r, t), b"batch too large"),
        # byte sizes that overflow: the arity is any 32-bit number until the context's rate is read, (2^32 - 1)^2 is below 2^64, and
        # k * depth * (arity - 1) * 32 bytes of openings at the largest k is about 2^70
        ((fake, 0xFFFFFFFF, 2, i, n, p, (1 << 32) - 2, w, r, t), b"overflows size_t"),
        ((fake, 0xFFFFFFFF, 1, i, n, p, (1 << 32) - 2, w, r, t), b"overflows size_t"),
    ]
    for args, needle in cases:
        assert fn(*args) == _lib.PMX_ERR_ARG, args
        assert needle in lib.pmx_last_error(), (needle, lib.pmx_last_error())
    for bad in ([16, 3], [3, U64], [1 << 63, 16]):
        ix = np.array(bad, dtype=np.uint64)
        assert fn(fake, 2, 4, _p(ix), n, p, 2, w, r, t) == _lib.PMX_ERR_ARG
        first = next(x for x in bad if x >= 16)
        assert b"leaf index %d out of range" % first in lib.pmx_last_error()
    assert (wit == 0x77).all() and (roots == 0x77).all() and (root == 0x77).all(), "a refusal wrote a result"
    # k = 0 with no root asked for: PMX_OK, nothing launched (no context is read), nothing written
    assert fn(fake, 2, 4, None, None, None, 0, w, r, None) == _lib.PMX_OK
    assert fn(fake, 2, 64, i, n, p, 0, None, None, None) == _lib.PMX_OK
    assert (wit == 0x77).all() and (roots == 0x77).all()


def test_the_entry_is_declared_exported_and_bound_and_adds_no_dev_entry():
    header = open(os.path.join(ROOT, "include", "poseidon_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\b" + ENTRY + r"\s*\(", code)
    assert ENTRY in _lib.SIGNATURES
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), ENTRY), path
    assert not re.search(r"\bpmx_merkle_update_witnesses\w*_dev\b", header)
    assert len(set(re.findall(r"\b(pmx_\w+_dev)\s*\(", code))) == 25        # the device entry points are what they were
    for sentence in ("no device-resident form", "no forest of matrices", "no device-group form", "no *_dev entry"):
        assert sentence in header
    assert "no leaf update of a fixed-depth tree" not in header and "pmx_merkle_ary_verify_paths" in header
    assert f"fn {ENTRY}(" in open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert "pub fn merkle_update_witnesses(" in open(os.path.join(ROOT, "bindings", "rust", "src", "mod.rs")).read()
    assert "merkle_update_witnesses(" in open(os.path.join(ROOT, "sponge_amd", "host", "poseidon_sponge.hpp")).read()
    import sponge_amd as S
    from sponge_amd.poseidon import Context
    assert callable(S.update_witnesses) and callable(Context.merkle_update_witnesses)
    assert _lib.lib().pmx_abi_version() == 5                                # additive: the ABI version stays
