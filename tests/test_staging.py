"""The layout of a host-buffer entry's device staging blocks as arithmetic (sponge_amd/csrc/pmx_staging.hpp; the call scope of
pmx_ctx.hpp hands a block out for one), on the CPU: the header compiled for the host behind tests/staging/staging_host.cpp.
- Every section starts on a 16-byte boundary, and the offsets are the running aligned sums.
- The overflow flag is set exactly when a product or the (aligned) sum exceeds SIZE_MAX.
- Every layout the entries of pmx_batch.cpp, pmx_sponge.cpp, pmx_matrix.cpp and pmx_merkle.cpp state comes out with the offsets their bodies computed by hand before
  the header existed: those expressions are written out here.
- tests/staging/sanitize_main.cpp, a program of its own, walks blocks of exactly bytes() bytes under ASan + UBSan."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sponge_amd", "csrc")
HERE = os.path.join(ROOT, "tests", "staging")
SIZE_MAX = 2 ** (8 * ctypes.sizeof(ctypes.c_size_t)) - 1
SMALL_CALL_BYTES = 64 * 1024


@pytest.fixture(scope="module")
def st(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("staging") / "libstaging_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-DPMX_HOSTCHECK", "-I", CSRC,
                           os.path.join(HERE, "staging_host.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    z, zp = ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)
    lib.st_layout.argtypes, lib.st_layout.restype = [zp, zp, z, zp, zp], ctypes.c_int
    lib.st_product.argtypes, lib.st_product.restype = [z, z, z, z, zp, zp], ctypes.c_int
    return lib


def layout(st, sections):
    """(offsets, bytes, overflowed) of sections [(count, elem_bytes), ...]"""
    n = len(sections)
    arr = ctypes.c_size_t * n
    offsets, total = arr(), ctypes.c_size_t()
    flag = st.st_layout(arr(*[c for c, _ in sections]), arr(*[e for _, e in sections]), n, offsets, ctypes.byref(total))
    return list(offsets), total.value, bool(flag)


def up16(x):
    return (x + 15) // 16 * 16


def test_sections_are_16_aligned_and_offsets_are_the_running_aligned_sums(st):
    for e1 in (1, 4, 8, 32):
        for e2 in (1, 3, 8, 96):
            for n1 in range(0, 41):
                for n2 in (0, 1, 2, 5, 16, 33):
                    sections = [(n1, e1), (n2, e2), (0, 32), (n1, 1), (3, 8)]
                    offsets, total, flag = layout(st, sections)
                    assert not flag
                    end, want = 0, []
                    for count, elem in sections:
                        want.append(up16(end))
                        end = want[-1] + count * elem
                    assert offsets == want and total == end, (sections, offsets, total)
                    assert all(o % 16 == 0 for o in offsets)
    assert layout(st, []) == ([], 0, False)
    assert layout(st, [(0, 32)]) == ([0], 0, False)          # an empty section is allowed, and the next starts where it does
    assert layout(st, [(0, 32), (5, 1)])[:2] == ([0, 0], 5)


@pytest.mark.parametrize("elem", [3, 8, 32, 96])
def test_the_flag_is_set_exactly_when_a_product_or_the_sum_exceeds_size_max(st, elem):
    most = SIZE_MAX // elem
    assert layout(st, [(most, elem)]) == ([0], most * elem, False)
    assert layout(st, [(most + 1, elem)])[2]
    assert layout(st, [(SIZE_MAX, elem)])[2]
    # the sum: a second section that just fits behind the first, and one byte more
    lead = 16 * elem
    assert layout(st, [(lead, 1), (SIZE_MAX - lead, 1)]) == ([0, lead], SIZE_MAX, False)
    assert layout(st, [(lead, 1), (SIZE_MAX - lead + 1, 1)])[2]
    # a sum that overflows only through the alignment padding: 16 + (SIZE_MAX - 31) + 1 + 14 = SIZE_MAX fits, but the last section would
    # have to start on the boundary behind SIZE_MAX - 14
    sections = [(16, 1), (SIZE_MAX - 31, 1), (1, 1)]
    assert layout(st, sections) == ([0, 16, SIZE_MAX - 15], SIZE_MAX - 14, False)
    assert sum(c * e for c, e in sections + [(14, 1)]) == SIZE_MAX
    assert layout(st, sections + [(14, 1)])[2]
    assert layout(st, sections + [(0, 1)])[2]                # even an empty section has no boundary left to start on
    assert not layout(st, [(16, 1), (SIZE_MAX - 31, 1), (15, 1)])[2]     # the same bytes without a boundary between them
    # a section counted in two factors
    off, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert st.st_product(200, most, 1, elem, ctypes.byref(off), ctypes.byref(total)) == 1    # 208 + most * elem does not fit
    assert st.st_product(0, most, 1, elem, ctypes.byref(off), ctypes.byref(total)) == 0 and total.value == most * elem
    assert st.st_product(0, 1 << 33, 1 << 31, elem, ctypes.byref(off), ctypes.byref(total)) == 1    # the product of the factors
    assert st.st_product(0, 1 << 33, 0, elem, ctypes.byref(off), ctypes.byref(total)) == 0 and total.value == 0
    assert st.st_product(5, 7, 3, elem, ctypes.byref(off), ctypes.byref(total)) == 0 and (off.value, total.value) == (16, 16 + 21 * elem)


# ---- the layouts of the entries, against the expressions their bodies had ---------------------------------------------------------------
def test_the_mode_words_sit_where_the_sponge_bodies_put_them(st):
    for t in (3, 9):
        for n in range(1, 41):
            st_bytes, words = n * t * 32, (n * 4 + 15) // 16 * 16
            # [states | tag | index]: ResidentSponges with an empty io section, closed by an empty section that ends it on a boundary
            offsets, total, flag = layout(st, [(st_bytes, 1), (0, 1), (n, 4), (n, 4), (0, 1)])
            assert not flag and offsets == [0, st_bytes, st_bytes, st_bytes + words, st_bytes + 2 * words]
            assert total == st_bytes + 2 * words
            # the packed [states | io | tag | index] of sponge_host
            for length in (0, 1, 3, 17):
                io_bytes = n * length * 32
                offsets, total, flag = layout(st, [(st_bytes, 1), (io_bytes, 1), (n, 4), (n, 4), (0, 1)])
                o_tag = st_bytes + io_bytes
                assert not flag and offsets == [0, st_bytes, o_tag, o_tag + words, o_tag + 2 * words]
                assert total == st_bytes + io_bytes + 2 * words          # the bytes the packed call copies each way


def test_the_packed_limit_falls_where_the_hand_written_size_put_it(st):
    # sponge_host packs when st_bytes + io_bytes + 2 * words <= 64 KiB: the layout's bytes(), its last section closed on a boundary
    for t, length in ((3, 3), (9, 8), (3, 0), (2, 1)):
        edge = SMALL_CALL_BYTES // (32 * (t + length) + 8)
        seen = set()
        for n in range(max(1, edge - 6), edge + 7):
            st_bytes, io_bytes, words = n * t * 32, n * length * 32, (n * 4 + 15) // 16 * 16
            total = layout(st, [(st_bytes, 1), (io_bytes, 1), (n, 4), (n, 4), (0, 1)])[1]
            old = st_bytes + io_bytes + 2 * words <= SMALL_CALL_BYTES
            assert total == st_bytes + io_bytes + 2 * words and (total <= SMALL_CALL_BYTES) == old, (t, length, n)
            seen.add(old)
        assert seen == {True, False}


def test_the_merkle_and_matrix_blocks_sit_where_their_bodies_put_them(st):
    for k in range(1, 13):
        for arity in range(2, 9):
            # [leaves | work]: d_work = d_leaves + k * 4 words, k * (arity + 2) * 32 bytes
            assert layout(st, [(k, 32), (k, (arity + 1) * 32)]) == ([0, k * 32], k * (arity + 2) * 32, False)
            for depth in range(0, 6):
                # paths [k][depth][arity - 1][4]
                assert layout(st, [(k, depth * (arity - 1) * 32)]) == ([0], k * depth * (arity - 1) * 32, False)
            # [rows | slots] of pmx_merkle_ary_update: d_slots = d_rows + n_rows * arity * 4 words, plan.upload.size() * 8 bytes
            assert layout(st, [(k, arity * 32), (k, 8)]) == ([0, k * arity * 32], (k * arity * 4 + k) * 8, False)
        # [root | indices]: d_idx = d_root + 4 words, 32 + k * 8 bytes
        assert layout(st, [(1, 32), (k, 8)]) == ([0, 32], 32 + k * 8, False)
        # [rows | ok] of pmx_matrix_verify_rows: d_ok = d3 + row_bytes, row_bytes + k bytes; the Merkle verifiers have no rows
        for row_len in (1, 3, 10):
            row_bytes = k * row_len * 32
            assert layout(st, [(k * row_len, 32), (k, 1)]) == ([0, row_bytes], row_bytes + k, False)
        assert layout(st, [(0, 32), (k, 1)]) == ([0, 0], k, False)
    for depth in range(1, 9):
        for arity in range(2, 9):
            # [e | rows] of pmx_merkle_fixed_defaults: row l at element depth + 1 + l * arity
            assert layout(st, [(depth + 1, 32), (depth, arity * 32)]) == ([0, (depth + 1) * 32], (depth + 1 + depth * arity) * 32, False)
    for t in range(2, 17):
        # [state | result] of pmx_sponge_grind: st_bytes + 16
        assert layout(st, [(t, 32), (2, 8)]) == ([0, t * 32], t * 32 + 16, False)


# ---- the header under the sanitizers: a program of its own, nothing sanitized is loaded into this process ----------------------------
def test_staging_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "staging_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-DPMX_HOSTCHECK", "-I", CSRC, os.path.join(HERE, "sanitize_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "sanitized ok" in out.stdout, out.stdout + out.stderr
