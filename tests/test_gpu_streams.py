"""Every single-device *_dev entry point of include/poseidon_mi355x.h on a side stream and - where the header allows it - under graph capture.

The header's contract for these calls is about streams: each takes a hipStream_t and only enqueues; some may be captured into a graph.  The
rest of the suite passes the null stream, on which a launch, memset or copy that goes to the wrong stream still runs in order.  Here the
stream is torch.cuda.Stream(device="cuda:0"), non-blocking with respect to the null stream; cases, buffers and the C port's answers come
from tests/streams_cases.py, one cell per entry point and engine (test_every_dev_entry_point_has_its_cells).

Part A, test_ordered_on_a_side_stream.  The buffers the call reads hold poison; the real inputs wait in staging tensors.  On the stream,
with no host synchronisation in between: a delay, an event, device-to-device copies of the inputs (indices, offsets and mode words
included), the call, copies of every out / inout buffer into result tensors.  Right after the call returns the event must still be
pending - otherwise the test FAILS as inconclusive, it never passes - and after the stream has drained the result copies equal the C port
in full.  A piece of the call on any other stream reads poison or is overtaken by the copy-out.  (Poisoned d_offsets are zeros, not random
words: a launch that read them early then absorbs empty rows - a wrong answer, never an address outside d_in.)  Every case first makes the
identical call once on the same stream with throw-away buffers: the pooled entries get their block (the measured call must not reach
hipMalloc), and for all of them the one-off host cost of a kernel's first launch in the process is not charged against the delay.
(What this cannot see: the memset that zeroes the pass form's counters, sent to another stream, runs EARLY here and the counters are
still zero when the kernels read them.  Making it run late would let the kernels append through stale counters, past their lists.)

The delay.  torch.cuda._sleep counts cycles of a device clock that is not specified, so it was measured on the MI355X: events around the
sleep, time.perf_counter around the enqueue alone (six calls of a case on an idle stream, the first - which pays for the kernel's first
launch in the process, 3 to 21 ms - left out).
    sleep:    1 000 000 cycles 0.42 ms, 5 000 000 cycles 2.09 ms, 20 000 000 cycles 8.34 ms: linear, 0.417 ms per million.
    enqueue:  t = 9 pass-form absorb (17 elements, 257 sponges) 0.020 to 0.050 ms; t = 9 varlen hash 0.048 to 0.060 ms; 2^17-leaf tree (17
              launches) 0.054 to 0.076 ms; arity-2 ragged update, k = 5 (28 launches) 0.084 to 0.094 ms; the slowest is the longest launch
              chain, not the pass form: arity-2 ragged verify_paths, depth 10 (a copy and 22 launches) 0.089 to 0.117 ms.
    chosen:   SLEEP_CYCLES = 50 000 000, about 21 ms: 180 times the slowest enqueue measured.  Ten times it would be 1.2 ms; the rest is
              room for a host thread that loses its CPU for a few milliseconds between the event and the end of the call, which would
              turn a correct run into an inconclusive one.  50 cases cost one second of delay.

Part B, test_captured_into_a_graph: exactly one call captured on the side stream (torch.cuda.graph, capture_error_mode="global", a linear
chain).  Capturing executes nothing (every buffer byte-identical to its clone); the replay gives the C port's answer for input set A; the
same buffers overwritten in place with set B - other values, other index contents, the same shapes - and replayed give the answer for B:
the graph holds pointers and shapes, no data seen at enqueue time.  The 2^17-leaf tree is replayed once, on A only.  The pass-form
drivers, the varlen entries and squeeze bytes / bits are NOT captured: the header forbids it (their per-stream pool may call hipMalloc),
and capturing them would only invalidate a capture.  test_cold_capture_in_a_fresh_process captures in a child process whose first launch
of a kernel of the library is the captured one (tests/streams_cold_worker.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from sponge_amd import _lib

import streams_cases as C

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLEEP_CYCLES = 50_000_000        # about 21 ms on the MI355X (module docstring)
ZERO_POISON = ("d_offsets",)

IDS = [C.case_id(c) for c in C.CASES]
CAPTURED = [c for c in C.CASES if c.entry in C.CAPTURABLE]


@pytest.fixture(scope="module")
def side():
    s = torch.cuda.Stream(device="cuda:0")
    yield s
    s.synchronize()


def _up(content):
    """a numpy array as a flat byte tensor on the device"""
    return torch.from_numpy(np.ascontiguousarray(content).reshape(-1).view(np.uint8).copy()).to("cuda:0")


def _poisoned(name, content, seed):
    if name in ZERO_POISON:
        return torch.zeros(content.nbytes, dtype=torch.uint8, device="cuda:0")
    return _up(C.poison(content.shape, content.dtype, seed))


def _equal(got, want, what):
    got = got.cpu().numpy().view(want.dtype).reshape(want.shape)
    if not np.array_equal(got, want):
        rows = np.nonzero((got.reshape(want.shape[0], -1) != want.reshape(want.shape[0], -1)).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(rows)} of {want.shape[0]} rows differ from the C port, first {rows[:8]}")


def _ok(rc, case):
    assert rc == _lib.PMX_OK, (C.case_id(case), rc, _lib.lib().pmx_last_error())


# ---- Part A ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_ordered_on_a_side_stream(case, side):
    C.assert_engines(case)
    bufs, want = C.data(case)
    reads = [n for n, (c, role) in bufs.items() if role in ("in", "inout")]
    staging = {n: _up(bufs[n][0]) for n in reads}
    dev = {n: _poisoned(n, c, 11 + i) for i, (n, (c, role)) in enumerate(bufs.items())}
    spare = {n: (staging[n].clone() if n in staging else _poisoned(n, c, 31 + i)) for i, (n, (c, role)) in enumerate(bufs.items())}
    result = {n: torch.empty_like(dev[n]) for n in want}
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _ok(C.invoke(case, spare, side), case)          # the identical call on throw-away buffers (module docstring)
        side.synchronize()
        torch.cuda.synchronize()
        torch.cuda._sleep(SLEEP_CYCLES)
        e_delay = torch.cuda.Event()
        e_delay.record(side)
        for n in reads:
            dev[n].copy_(staging[n], non_blocking=True)
        rc = C.invoke(case, dev, side)
        delay_over = e_delay.query()
        for n in want:
            result[n].copy_(dev[n], non_blocking=True)
    side.synchronize()
    _ok(rc, case)
    if delay_over:
        pytest.fail("delay too short: inconclusive")
    for n in want:
        _equal(result[n], want[n], (C.case_id(case), n))
    torch.cuda.synchronize()
    for n in want:                                      # and nothing arrived after the copy-out
        assert torch.equal(result[n], dev[n]), (C.case_id(case), n, "changed after the copy-out")


# ---- Part B ---------------------------------------------------------------------------------------------------------------------------------
def _load(dev, bufs):
    for n, (content, role) in bufs.items():
        dev[n].copy_(_up(content))
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", CAPTURED, ids=[C.case_id(c) for c in CAPTURED])
def test_captured_into_a_graph(case, side):
    C.assert_engines(case)
    bufs, want = C.data(case)
    dev = {n: _up(c) for n, (c, role) in bufs.items()}              # out and scratch buffers come poisoned from the case
    torch.cuda.synchronize()
    before = {n: t.clone() for n, t in dev.items()}
    g, rc = torch.cuda.CUDAGraph(), None
    try:
        with torch.cuda.graph(g, stream=side, capture_error_mode="global"):
            rc = C.invoke(case, dev, side)
    except RuntimeError as exc:
        pytest.fail(f"{C.case_id(case)}: the capture failed (status {rc}, {_lib.lib().pmx_last_error()}): {exc}")
    _ok(rc, case)
    torch.cuda.synchronize()
    for n in dev:
        assert torch.equal(before[n], dev[n]), (C.case_id(case), n, "capturing executed something")
    g.replay()
    torch.cuda.synchronize()
    for n in want:
        _equal(dev[n], want[n], (C.case_id(case), n, "replay on input set A"))
    if C.is_big(case):
        return
    bufs_b, want_b = C.data(case, 1)
    same_tree = ("d_root",) + (("d_nodes",) if case.entry.endswith(("paths_dev", "update_dev")) else ())     # A and B open / update one tree
    assert all(not np.array_equal(bufs[n][0], bufs_b[n][0]) for n in bufs if n not in same_tree), "input set B must differ from A"
    _load(dev, bufs_b)                                               # in place: the same device buffers, outputs poisoned again
    g.replay()
    torch.cuda.synchronize()
    for n in want_b:
        _equal(dev[n], want_b[n], (C.case_id(case), n, "replay on input set B"))


def test_cold_capture_in_a_fresh_process(tmp_path):
    """the parent leaves inputs and the C port's answers as .npy files; the child (tests/streams_cold_worker.py) reads nothing else"""
    permute = next(c for c in C.CASES if c.entry == "pmx_permute_batch_dev" and c.label == "t3" and dict(c.shape)["n"] == 257)
    tree = next(c for c in C.CASES if c.entry == "pmx_merkle_2to1_dev" and c.label == "t3" and dict(c.shape)["n_leaves"] == 512)
    for case, names in ((permute, ("states", "permuted")), (tree, ("first", "nodes"))):
        bufs, want = C.data(case)
        (content, role), = bufs.values()
        np.save(tmp_path / (names[0] + ".npy"), content)
        np.save(tmp_path / (names[1] + ".npy"), next(iter(want.values())))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "streams_cold_worker.py"), str(tmp_path)], capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0 and "cold capture ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- the tables -------------------------------------------------------------------------------------------------------------------------------
def test_every_dev_entry_point_has_its_cells():
    """the case tables against the *_dev functions the header declares and the library exports: each is run on a side stream, and captured
    when the header allows it, or is listed with the reason why not; and each runs on every engine cell of its family"""
    header = open(os.path.join(ROOT, "include", "poseidon_mi355x.h")).read()
    declared = set(re.findall(r"^int (pmx_\w+_dev)\(", header, flags=re.M))
    assert len(declared) == 25, sorted(declared)
    lib = _lib.lib()
    assert all(hasattr(lib, name) for name in declared), [name for name in declared if not hasattr(lib, name)]
    assert declared == {name for name in _lib.SIGNATURES if name.endswith("_dev")}
    on_stream = {c.entry for c in C.CASES}
    assert on_stream | set(C.OUT_OF_SCOPE) == declared and not on_stream & set(C.OUT_OF_SCOPE)
    assert {c.entry for c in CAPTURED} == set(C.CAPTURABLE)
    assert set(C.CAPTURABLE) | set(C.NOT_CAPTURABLE) == on_stream and not set(C.CAPTURABLE) & set(C.NOT_CAPTURABLE)
    assert all(C.OUT_OF_SCOPE.values()) and all(C.NOT_CAPTURABLE.values())
    cells = {}
    for case in C.CASES:
        cells.setdefault(case.entry, set()).update(C.assert_engines(case))
    batch = {"quad-t3", "window-t3", "t9-bn254"}
    tree = {"pmx_merkle_2to1_dev", "pmx_merkle_2to1_forest_dev"}
    for entry in on_stream:
        if entry in ("pmx_permute_batch_dev", "pmx_hash_batch_dev"):
            assert cells[entry] == batch | {"lds-t16"}, (entry, cells[entry])
        elif entry in C.NOT_CAPTURABLE or entry in tree:
            assert cells[entry] == batch, (entry, cells[entry])
        elif entry.endswith("paths_dev") and "verify" not in entry:
            assert cells[entry] == set(), entry          # a gather: no permutation engine
        elif "ragged" in entry or entry == "pmx_merkle_verify_paths_dev":
            assert cells[entry] == {"quad-t3", "t9-bn254"}, (entry, cells[entry])
        else:
            assert cells[entry] == {"t9-bn254"}, (entry, cells[entry])
    # the shapes the multi-launch entries need: both branches of the updates, both values of d_ok
    for entry in ("pmx_merkle_ary_update_dev", "pmx_merkle_ragged_update_dev"):
        for case in (c for c in C.CASES if c.entry == entry):
            s = dict(case.shape)
            parents = -(-s["n_leaves"] // s["arity"])
            assert s["k"] == 5 or s["k"] >= parents
        assert {dict(c.shape)["k"] == 5 for c in C.CASES if c.entry == entry} == {True, False}
