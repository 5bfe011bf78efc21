"""Every single-device entry point under injected HIP failures: what the header promises about the paths that nothing else runs.

The test library counts the checked HIP calls of the calling thread and fails the armed one in place of making it (pmx::hip_inject,
include/poseidon_mi355x_testing.h; the detector itself is tests/test_hip_inject_host.py).  An injected failure is a return value made on
the host: the entry leaves through its ordinary error path, nothing reaches the device that a clean call would not send.  For a case with
K checked calls EVERY k = 1 .. K is failed once, and after each
  - the call returned PMX_ERR_HIP and pmx_last_error() says "injected" - or, where the product absorbs the failure by design (the event
    of a pass-scratch block that cannot be recorded, a registration that falls back), PMX_OK with the exact result;
  - every guard and every input buffer of the host arena is unchanged, and states / tag / index of the absorb, squeeze and varlen entries;
  - pmx_stream_synchronize(0, NULL) returns PMX_OK and no block of the pass-scratch pool is held;
  - the same case called again, unarmed, on the same context returns PMX_OK and is byte for byte the C port's answer: the lock was released,
    the streams drained, the staging blocks and the pool are usable.
A PMX_ERR_HIP whose message is not the injected one ends the session (the device may have faulted), as in tests/test_gpu_host_footprint.py,
whose case builders, boxes and 5-unit shapes these are.

Cold sweep: a fresh context per k, so that the allocations of a first call (staging blocks, the page-locked block, pool blocks) are among
the calls failed.  Warm sweep, at shapes of several passes, slabs, pieces and chunks: one context, so that a failure lands between pieces
and behind work already enqueued on blocks an earlier call grew.  The K of every case is printed (pytest -s) and asserted <= 200."""
import ctypes
import functools
import os

import numpy as np
import pytest

from sponge_amd import _lib, synth
from sponge_amd.poseidon import c_config
from oracle import cref
from oracle import poseidon_oracle as O

import sponge_amd as S
import host_arena as H
import merkle_ary_oracle as M
import streams_cases as SC
import test_gpu_host_footprint as HF

pytestmark = pytest.mark.gpu

OK, ERR_HIP = _lib.PMX_OK, _lib.PMX_ERR_HIP
FAR = 1 << 40                            # a count no call reaches
K_MAX = 200
_fn = HF._fn
SPONGE_FAMILY = {"pmx_sponge_absorb_batch", "pmx_sponge_squeeze_batch", "pmx_sponge_squeeze_bytes_batch", "pmx_sponge_squeeze_bits_batch",
                 "pmx_sponge_absorb_varlen_batch"}
ABSORBED = ("hipEventRecord(b.done", "hipHostRegister(")      # failures the product absorbs: the call goes on and must be right


def last_error():
    return _fn("pmx_last_error")() or b""


def arm(k):
    assert _fn("pmx_test_fail_hip")(k) == OK


def disarm():
    """(calls since the arm, the text of the failure made since, b"" if none)"""
    calls, fired = _fn("pmx_test_hip_calls")(), _fn("pmx_test_hip_fired")() or b""
    arm(0)
    return calls, fired.decode()


def only_injected(rc, what):
    """a PMX_ERR_HIP that the injector did not make: nothing more is started on the device in this session"""
    if rc == ERR_HIP and b"injected" not in last_error():
        arm(0)
        pytest.exit(f"{what}: PMX_ERR_HIP: {last_error()}", returncode=3)


def pool(ctx):
    blocks, held, poisoned = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    assert _fn("pmx_test_pass_pool")(ctx, ctypes.byref(blocks), ctypes.byref(held), ctypes.byref(poisoned)) == OK
    return blocks.value, held.value, poisoned.value


def settled(ctx, what):
    rc = _fn("pmx_stream_synchronize")(0, None)
    only_injected(rc, what)
    assert rc == OK, (what, last_error())
    assert pool(ctx)[1] == 0, (what, "a pass-scratch block is still held")


class Context:
    """a context of the test library for one config, destroyed on the way out"""

    def __init__(self, cfg):
        self.c, self.handle = c_config(cfg), ctypes.c_void_p()

    def __enter__(self):
        rc = _fn("pmx_ctx_create")(ctypes.byref(self.c), 0, ctypes.byref(self.handle))
        only_injected(rc, "pmx_ctx_create")
        assert rc == OK, last_error()
        return self.handle

    def __exit__(self, *exc):
        assert _fn("pmx_ctx_destroy")(self.handle) == OK


@pytest.fixture(scope="module", params=list(HF.ARITY))
def box(request):
    """the footprint test's box without a context of its own: every sweep makes its contexts"""
    f, cfg, cr = M.config(request.param)
    yield HF.Box(request.param, f, cfg, cr, HF.ARITY[request.param], None, _fn)
    for hook in ("pmx_test_matrix_slab_rows", "pmx_test_merkle_fixed_piece", "pmx_test_grind_chunk"):
        _fn(hook)(0)
    arm(0)


# ---- host-buffer entries ------------------------------------------------------------------------------------------------------------------
class Arena:
    """one pageable guard-band arena of a case, refilled to the same image before every call"""

    def __init__(self, case):
        self.case, self.fn = case, _fn(case.entry)
        self.a = H.HostArena(case.buffers, 1)
        for name, data in case.inputs.items():
            self.a.put(name, data)
        self.initial = self.a.image.copy()

    def call(self, ctx):
        self.a.image[:] = self.initial
        self.a.snapshot()
        case, a = self.case, self.a
        return self.fn(ctx, *case.args(lambda name: None if name in case.null else ctypes.c_void_p(a.ptr(name))))

    def exact(self, what):
        for name, want in self.case.expected.items():
            assert self.a.get(name, np.uint8).tobytes() == np.ascontiguousarray(want).tobytes(), (what, name)
        self.a.finish(self.case.written)

    def clean(self, ctx, what):
        """an unarmed call: PMX_OK and the C port's bytes"""
        rc = self.call(ctx)
        only_injected(rc, what)
        assert rc == OK, (what, rc, last_error())
        assert H.guard_holds(self.a.plan)
        self.exact(what)

    def failed(self, ctx, k, what):
        """the call with its k-th checked HIP call failed, and everything that must hold behind it"""
        arm(k)
        rc = self.call(ctx)
        calls, fired = disarm()
        what = (*what, k, fired)
        only_injected(rc, what)
        assert fired.startswith("injected in place of ") and calls >= k, (what, calls)
        if any(site in fired for site in ABSORBED):
            assert rc == OK, (what, rc, last_error())
            self.exact(what)
        else:
            assert rc == ERR_HIP and b"injected" in last_error(), (what, rc, last_error())
            assert fired.encode() in last_error(), (what, last_error())          # the expression text of the call that was not made
            self.a.finish(None)                                                   # guards and inputs; an output may hold anything inside its bounds
            if self.case.entry in SPONGE_FAMILY:
                for name in ("states", "mode_tag", "mode_index"):
                    r = self.a.plan[name]
                    assert np.array_equal(self.a.before[r.offset:r.offset + r.nbytes], self.a.image[r.offset:r.offset + r.nbytes]), (what, name)
        settled(ctx, what)

    def count(self, ctx, what):
        """K: the checked calls of a clean call"""
        arm(FAR)
        rc = self.call(ctx)
        calls, fired = disarm()
        only_injected(rc, what)
        assert rc == OK and fired == "", (what, rc, last_error())
        self.exact(what)
        assert 0 < calls <= K_MAX, (what, calls)
        return calls


def cold_sweep(b, case):
    arena, what = Arena(case), (case.entry, b.label, "cold")
    with Context(b.cfg) as ctx:
        K = arena.count(ctx, what)
    for k in range(1, K + 1):
        with Context(b.cfg) as ctx:
            arena.failed(ctx, k, what)
            arena.clean(ctx, (*what, k, "again"))
    print(f"K[{case.entry}, {b.label}, cold] = {K}")
    return K


def warm_sweep(b, case):
    arena, what = Arena(case), (case.entry, b.label, "warm")
    with Context(b.cfg) as ctx:
        arena.clean(ctx, what)                                   # grows the blocks
        K = arena.count(ctx, what)
        for k in range(1, K + 1):
            arena.failed(ctx, k, what)
            arena.clean(ctx, (*what, k, "again"))
        assert arena.count(ctx, what) == K                       # the sweep left the context as warm as it found it
    print(f"K[{case.entry}, {b.label}, warm] = {K}")
    return K


def two_ary(b):
    return b._replace(arity=2)


def small_cases(b):
    """{key of host_arena.entry_point_buffers: case}: every host-buffer entry that reaches the device, at the footprint test's 5-unit shape"""
    r, a, ABSORBING = b.cfg.rate, b.arity, _lib.MODE_ABSORBING
    cases = {
        "pmx_permute_batch": HF.permute_case(b.label, 5),
        "pmx_hash_batch": HF.hash_case(b.label, 5, r + 1, 2),
        "pmx_sponge_absorb_batch": HF.absorb_case(b, 5, 3),
        "pmx_sponge_squeeze_batch": HF.squeeze_case(b, 5, 3),
        "pmx_sponge_squeeze_bytes_batch": HF.squeeze_cut_case(b, 5, 5, False),
        "pmx_sponge_squeeze_bits_batch": HF.squeeze_cut_case(b, 5, 9, True),
        "pmx_sponge_grind": HF.grind_case(b, 1, ABSORBING, 1, 3, 1000, 50),
        "pmx_merkle_ary_update": HF.update_case(b, 3, 5),
        "pmx_merkle_frontier_append": HF.append_case(b, 4, 3, 5, False, True),
        "pmx_merkle_frontier_append (aliased)": HF.append_case(b, 4, 3, 5, True, True),
        "pmx_merkle_update_witnesses": HF.witness_case(b.label, HF.witness_arities(b)[0], 6, 5),
        "pmx_matrix_verify_rows": HF.verify_rows_case(b, 11, 3, 5),
    }
    cases["pmx_sponge_absorb_varlen_batch"], cases["pmx_hash_varlen_batch"] = HF.varlen_cases(b, 5)
    cases["pmx_merkle_fixed"], cases["pmx_merkle_fixed_defaults"] = HF.fixed_cases(b, 4, 5)
    cases["pmx_matrix_leaves"], cases["pmx_matrix_commit"] = HF.matrix_cases(b, 5, 2 * r + 1, HF.ROW)
    # the builders and verifiers at the box's arity, the 2-to-1 ones at arity 2 on either box
    for case in HF.builder_cases(b, 3, (True, True)) + HF.verify_cases(b, 5, False):
        cases[case.entry] = case
    if a != 2:
        for case in HF.builder_cases(two_ary(b), 3, (True, True)) + HF.verify_cases(two_ary(b), 5, False):
            if "2to1" in case.entry or case.entry == "pmx_merkle_verify_paths":
                cases[case.entry] = case
    return cases


# what of the table never makes a HIP call (host-only gathers and arithmetic) or belongs to the device groups (pmx_mgpu.cpp: out of scope)
NO_HIP_CALL = {"pmx_merkle_paths", "pmx_merkle_ary_paths", "pmx_merkle_ragged_paths", "pmx_merkle_fixed_paths", "pmx_matrix_rows",
               "pmx_find_poseidon_ark_and_mds", "pmx_mont_constants", "pmx_to_mont", "pmx_from_mont", "pmx_merkle_ary_shape",
               "pmx_merkle_ragged_shape", "pmx_merkle_fixed_shape", "pmx_shard_bounds"}
ENTRIES = sorted(name for name in H.entry_point_buffers() if name not in NO_HIP_CALL and not name.startswith("pmx_mgpu_"))


def test_the_sweeps_cover_the_table_of_host_buffer_entries(box):
    """the table that tests/test_host_arena_table.py counts against the header's prototypes: every entry of it that is not host-only or a
    device group's has a case here, and the footprint test has one for exactly the same entries"""
    assert sorted(small_cases(box)) == ENTRIES and len(ENTRIES) == 26
    source = open(HF.__file__).read()
    for name in ENTRIES:
        assert f'"{name.split(" ")[0]}"' in source, name


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_checked_call_of_a_small_call_failed_once(box, entry):
    cold_sweep(box, small_cases(box)[entry])


def several_pieces(b, which):
    """the warm sweep's shapes: at least three listed passes, slabs, pieces, chunks or levels"""
    r, depth = b.cfg.rate, 12 if b.arity == 2 else 6
    if which in ("absorb", "squeeze"):                        # one sponge more than the packed block holds: the resident walk; 2 rate + 1 elements
        n = HF.packed_limit(b.cfg.t, 2 * r + 1) + 1
        return (HF.absorb_case if which == "absorb" else HF.squeeze_case)(b, n, 2 * r + 1)
    if which == "matrix_commit":                              # 300 rows in slabs of 128
        assert b.fn("pmx_test_matrix_slab_rows")(128) == OK
        return HF.matrix_cases(b, 300, 5, HF.ROW)[1]
    if which == "frontier_append":                            # 300 leaves in pieces of 128
        assert b.fn("pmx_test_merkle_fixed_piece")(128) == OK
        return HF.append_case(b, depth, 7, 300, True, True)
    if which == "update_witnesses":                           # three levels, the slab of a level above the small-call limit
        a = HF.witness_arities(b)[0]
        return HF.witness_case(b.label, a, 3, HF.first_above((a - 1) * 32))
    assert which == "grind"                                   # 50 candidates in chunks of 20, nothing found: every chunk is walked
    assert b.fn("pmx_test_grind_chunk")(20) == OK
    return HF.grind_case(b, 1, _lib.MODE_SQUEEZING, 0, 40, 1000, 50)


@pytest.mark.parametrize("which", ["absorb", "squeeze", "matrix_commit", "frontier_append", "update_witnesses", "grind"])
def test_every_checked_call_of_a_call_of_several_pieces_failed_once(box, which):
    if which in ("absorb", "squeeze") and box.label != "t9-bn254":
        return                                                # the listed passes are the window engine's
    try:
        warm_sweep(box, several_pieces(box, which))
    finally:
        for hook in ("pmx_test_matrix_slab_rows", "pmx_test_merkle_fixed_piece", "pmx_test_grind_chunk"):
            box.fn(hook)(0)


# ---- the *_dev entries that take scratch from the per-stream pool --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hip():
    """the HIP runtime this process already holds, by its SONAME"""
    HF._library()
    mapped = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert mapped, "the test library maps a HIP runtime"
    name = mapped[0].rsplit("/", 1)[-1]
    soname = ".".join(name.split(".")[:3])                        # libamdhip64.so.N
    for candidate in (soname, mapped[0]):
        try:
            return ctypes.CDLL(candidate, mode=os.RTLD_NOW | os.RTLD_NOLOAD)      # the one already loaded, never a second runtime
        except OSError:
            continue
    raise AssertionError(f"the HIP runtime mapped at {mapped[0]} cannot be opened again")


class Stream:
    def __enter__(self):
        self.handle = ctypes.c_void_p()
        assert hip().hipStreamCreate(ctypes.byref(self.handle)) == 0
        return self.handle

    def __exit__(self, *exc):
        assert hip().hipStreamDestroy(self.handle) == 0


POOLED = [c for c in SC.CASES if c.entry in SC.NOT_CAPTURABLE and dict(c.shape)["n"] == 257]


class DeviceCase:
    """the buffers of a case of tests/streams_cases.py in device memory of their own, refilled before every call"""

    def __init__(self, case):
        self.case, self.fn = case, _fn(case.entry)
        self.bufs, self.want = SC.data(case)
        self.d = {}
        for name, (content, role) in self.bufs.items():
            p = ctypes.c_void_p()
            assert _fn("pmx_device_alloc")(0, ctypes.byref(p), content.nbytes) == OK
            self.d[name] = p

    def close(self):
        for p in self.d.values():
            assert _fn("pmx_device_free")(0, p) == OK

    def load(self, stream):
        """the inputs up on `stream`, and waited for (the sources are pageable)"""
        for name, (content, role) in self.bufs.items():
            assert _fn("pmx_device_upload")(0, self.d[name], content.ctypes.data, content.nbytes, stream) == OK
        assert _fn("pmx_stream_synchronize")(0, stream) == OK

    def call(self, ctx, stream, k=0):
        """fresh inputs, then the entry on `stream` (enqueue only) with its k-th checked call failed (0: none): the status"""
        self.load(stream)
        arm(k)
        s, d, r = dict(self.case.shape), self.d, SC._rate(self.case.label)
        e, n = self.case.entry, s["n"]
        sponge = (d.get("d_states"), d.get("d_mode_tag"), d.get("d_mode_index"))
        if e == "pmx_sponge_absorb_batch_dev":
            return self.fn(ctx, *sponge, d["d_in"], s["in_len"], n, stream)
        if e == "pmx_sponge_squeeze_batch_dev":
            return self.fn(ctx, *sponge, d["d_out"], s["out_len"], n, stream)
        if e == "pmx_sponge_absorb_varlen_batch_dev":
            return self.fn(ctx, *sponge, d["d_in"], d["d_offsets"], 5 * r, n, stream)
        if e == "pmx_hash_varlen_batch_dev":
            return self.fn(ctx, d["d_in"], d["d_offsets"], 5 * r, d["d_out"], s["out_len"], n, stream)
        assert e in ("pmx_sponge_squeeze_bytes_batch_dev", "pmx_sponge_squeeze_bits_batch_dev")
        return self.fn(ctx, *sponge, d["d_out"], s["length"], n, stream)

    def exact(self, stream, what):
        assert _fn("pmx_stream_synchronize")(0, stream) == OK, (what, last_error())
        for name, want in self.want.items():
            got = np.empty(want.nbytes, dtype=np.uint8)
            assert _fn("pmx_device_download")(0, got.ctypes.data, self.d[name], got.nbytes, stream) == OK
            assert _fn("pmx_stream_synchronize")(0, stream) == OK
            assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (what, name)

    def clean(self, ctx, stream, what):
        rc = self.call(ctx, stream)
        only_injected(rc, what)
        assert rc == OK, (what, rc, last_error())
        self.exact(stream, what)


@pytest.mark.parametrize("case", POOLED, ids=SC.case_id)
def test_every_checked_call_of_a_pooled_dev_entry_failed_once(case):
    f, cfg, cr = M.config(case.label)
    dev, what = DeviceCase(case), (case.entry, case.label)
    try:
        with Stream() as first, Stream() as second:
            with Context(cfg) as ctx:
                K = count_dev(dev, ctx, first, what)              # of a first call on a fresh context: the pool's allocations among them
            for k in range(1, K + 1):
                with Context(cfg) as ctx:
                    rc = dev.call(ctx, first, k)
                    calls, fired = disarm()
                    only_injected(rc, (*what, k))
                    assert fired.startswith("injected in place of "), (what, k, calls)
                    assert _fn("pmx_stream_synchronize")(0, first) == OK
                    blocks, held, poisoned = pool(ctx)
                    assert held == 0, (what, k, fired)
                    if any(site in fired for site in ABSORBED):
                        assert rc == OK and poisoned == 1, (what, k, fired, rc, poisoned)
                        dev.exact(first, (*what, k, fired))
                    else:
                        assert rc == ERR_HIP and b"injected" in last_error() and poisoned == 0, (what, k, fired, rc, last_error())
                    dev.clean(ctx, second, (*what, k, fired, "second stream"))
                    dev.clean(ctx, first, (*what, k, fired, "first stream again"))
                    assert pool(ctx)[1] == 0
        print(f"K[{case.entry}, {case.label}] = {K}")
    finally:
        arm(0)
        dev.close()


def count_dev(dev, ctx, stream, what):
    """the checked calls of the entry on a fresh context"""
    rc = dev.call(ctx, stream, FAR)
    K, fired = disarm()
    only_injected(rc, what)
    assert rc == OK and fired == "", (what, rc, last_error())
    dev.exact(stream, what)
    assert 0 < K <= K_MAX, (what, K)
    return K


def test_a_pool_block_whose_event_could_not_be_recorded_goes_to_no_other_stream():
    """the hipEventRecord of ctx_pass_done fails: the call itself succeeds, the block is poisoned, and a call of equal size on another
    stream gets a block of its own"""
    case = next(c for c in POOLED if c.entry == "pmx_sponge_absorb_batch_dev" and c.label == "t9-bn254")
    f, cfg, cr = M.config(case.label)
    dev = DeviceCase(case)
    try:
        with Stream() as first, Stream() as second:
            with Context(cfg) as ctx:
                K = count_dev(dev, ctx, first, case.entry)
            site = None
            for k in range(1, K + 1):                             # the ordinal of the record, by its expression text
                with Context(cfg) as ctx:
                    rc = dev.call(ctx, first, k)
                    calls, fired = disarm()
                    only_injected(rc, (case.entry, k))
                    assert _fn("pmx_stream_synchronize")(0, first) == OK
                    if "hipEventRecord(b.done" not in fired:
                        continue
                    site = k
                    assert rc == OK, last_error()                 # the case itself is not allowed to fail
                    assert pool(ctx) == (1, 0, 1)
                    dev.exact(first, "the call whose record failed")
                    other = DeviceCase(case)                      # a call of equal size on another stream, the first one's buffers left alone
                    try:
                        other.clean(ctx, second, "the call on the other stream")
                        assert pool(ctx) == (2, 0, 1)             # a different block
                        dev.exact(first, "the first call, behind the second")
                    finally:
                        other.close()
            assert site is not None, "no checked call of the case was the record of ctx_pass_done"
    finally:
        arm(0)
        dev.close()


# ---- a registration that fails ---------------------------------------------------------------------------------------------------------------
def registered(p):
    flags = ctypes.c_uint()
    rc = hip().hipHostGetFlags(ctypes.byref(flags), ctypes.c_void_p(p))
    if rc != 0:
        hip().hipGetLastError()
    return rc == 0


def test_a_failed_registration_leaves_the_buffer_as_it_is_and_the_call_still_answers():
    """pmx_permute_batch on a pageable buffer of just over ScopedPin::kMinBytes with its hipHostRegister failed: PMX_OK on the unpinned
    path, exact on 4096 rows (the first and last 256 among them), nothing left registered; and again unarmed, registered for the call"""
    label = "t3"
    f, cfg, cr = M.config(label)
    row = cfg.t * 32
    n = HF.PIN_MIN // row + 1
    assert (n - 1) * row < HF.PIN_MIN <= n * row
    states = synth.random_elements(f, n * cfg.t, seed=0xF411).reshape(n, cfg.t, 4)
    rng = np.random.default_rng(5)
    sample = np.concatenate([np.arange(256), np.sort(rng.choice(np.arange(256, n - 256), 4096 - 512, replace=False)), np.arange(n - 256, n)])
    assert sample.size == 4096 and (sample[:256] == np.arange(256)).all() and (sample[-256:] == np.arange(n - 256, n)).all()
    want = cr.permute_batch(np.ascontiguousarray(states[sample]), threads=0)
    case = HF.Case("pmx_permute_batch", H.permute_buffers(cfg.t, n), {"states": states}, {}, lambda p: (p("states"), n))
    arena = Arena(case)

    def exact(what):
        got = arena.a.get("states").reshape(n, cfg.t, 4)
        assert np.array_equal(got[sample], want), what
        arena.a.finish(None)
        assert not registered(arena.a.ptr("states")), what

    with Context(cfg) as ctx:
        assert not registered(arena.a.ptr("states"))
        arm(FAR)
        rc = arena.call(ctx)
        K, fired = disarm()
        only_injected(rc, "pmx_permute_batch, 16 MiB")
        assert rc == OK and fired == "" and 0 < K <= K_MAX, (rc, last_error(), K)
        exact("clean")
        site = None
        for k in range(1, K + 1):                                 # the registration's ordinal, by its expression text
            arm(k)
            rc = arena.call(ctx)
            calls, fired = disarm()
            only_injected(rc, ("pmx_permute_batch, 16 MiB", k))
            if "hipHostRegister(" not in fired:
                assert rc == ERR_HIP and b"injected" in last_error(), (k, fired, rc)
                assert not registered(arena.a.ptr("states")), (k, fired)
                settled(ctx, (k, fired))
                continue
            site = k
            assert rc == OK, (k, last_error())
            exact("the call whose registration failed")
            rc = arena.call(ctx)
            only_injected(rc, "pmx_permute_batch, 16 MiB, again")
            assert rc == OK, last_error()
            exact("the call behind it")
            break
        assert site is not None, "no checked call of the 16 MiB permutation was a registration"
        print(f"K[pmx_permute_batch, {label}, 16 MiB] = {K}, hipHostRegister is call {site}")


# ---- contexts and their cache ----------------------------------------------------------------------------------------------------------------
def permutes_exactly(ctx, f, cfg, cr):
    states = synth.random_elements(f, 5 * cfg.t, seed=77).reshape(5, cfg.t, 4)
    case = HF.Case("pmx_permute_batch", H.permute_buffers(cfg.t, 5), {"states": states}, {"states": cr.permute_batch(states, threads=0)},
                   lambda p: (p("states"), 5))
    Arena(case).clean(ctx, "5 states on the context")


def test_every_checked_call_of_ctx_create_failed_once(box):
    c, create = c_config(box.cfg), _fn("pmx_ctx_create")
    handle = ctypes.c_void_p()
    arm(FAR)
    rc = create(ctypes.byref(c), 0, ctypes.byref(handle))
    K, fired = disarm()
    only_injected(rc, "pmx_ctx_create")
    assert rc == OK and handle.value and 0 < K <= K_MAX
    assert _fn("pmx_ctx_destroy")(handle) == OK
    for k in range(1, K + 1):
        handle = ctypes.c_void_p(1)
        arm(k)
        rc = create(ctypes.byref(c), 0, ctypes.byref(handle))
        calls, fired = disarm()
        only_injected(rc, ("pmx_ctx_create", k))
        assert rc == ERR_HIP and b"injected" in last_error() and fired.encode() in last_error(), (k, rc, last_error())
        assert handle.value is None, (k, "*out is not NULL")
    with Context(box.cfg) as ctx:
        permutes_exactly(ctx, box.f, box.cfg, box.cr)
    print(f"K[pmx_ctx_create, {box.label}] = {K}")


def test_every_checked_call_of_ctx_acquire_failed_once(box):
    """a config no other test acquires (partial rounds of its own): not in the cache before, and in it after no failure"""
    field, rate, alpha, rf, rp = M.CONFIGS[box.label]
    f, p, bits = M.FIELD[field]
    rp += 2
    cfg, cr = S.poseidon_config_from_lfsr(f, rate, alpha, rf, rp), cref.CRef(O.make_config(p, bits, rate, alpha, rf, rp))
    c, acquire, release = c_config(cfg), _fn("pmx_ctx_acquire"), _fn("pmx_ctx_release")

    def built():
        """an unarmed acquire that builds a context, a second one that finds it, both handed back and the cache emptied"""
        first, second = ctypes.c_void_p(), ctypes.c_void_p()
        arm(FAR)
        rc = acquire(ctypes.byref(c), 0, ctypes.byref(first))
        calls, fired = disarm()
        only_injected(rc, "pmx_ctx_acquire")
        assert rc == OK and first.value and calls > 0, (rc, last_error(), calls)       # (a context found in the cache costs no HIP call)
        arm(FAR)
        assert acquire(ctypes.byref(c), 0, ctypes.byref(second)) == OK and second.value == first.value
        assert disarm()[0] == 0
        return first, calls

    def handed_back(handle):
        assert release(handle) == OK and release(handle) == OK
        assert _fn("pmx_ctx_cache_clear")() == OK

    handle, K = built()
    assert K <= K_MAX
    permutes_exactly(handle, f, cfg, cr)
    handed_back(handle)
    for k in range(1, K + 1):
        handle = ctypes.c_void_p(1)
        arm(k)
        rc = acquire(ctypes.byref(c), 0, ctypes.byref(handle))
        calls, fired = disarm()
        only_injected(rc, ("pmx_ctx_acquire", k))
        assert rc == ERR_HIP and b"injected" in last_error() and handle.value is None, (k, rc, last_error())
        handle, again = built()                                   # the failure left no entry behind: this acquire built one
        assert again == K, (k, again)
        handed_back(handle)
    handle, _ = built()
    permutes_exactly(handle, f, cfg, cr)
    handed_back(handle)
    print(f"K[pmx_ctx_acquire, {box.label}] = {K}")
