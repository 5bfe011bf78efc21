"""squeeze_bytes / squeeze_bits of device-resident batches (pmx_sponge_squeeze_{bytes,bits}_batch_dev) against the native squeeze they
are built on, and the host entry against what a caller did before it existed.  BLS12-381 Fr t = 3 at 2^20 sponges and BN254 Fr t = 9 at
2^18, all Absorbing, 32 bytes / 256 bits per sponge (E = 2 native elements).
  dev:   every step = restore the sponges (device-to-device copies) + the call, timed by HIP events on the launch stream; the restore alone
         is timed the same way and subtracted; median of the steps after a warm-up.  The ratio's denominator is
         pmx_sponge_squeeze_batch_dev(out_len = 2) on the same sponges, and - with --baseline-library PATH - the same entry of ANOTHER
         build of the library (the parent commit's), measured by a child process of this run (that entry is unchanged, so the parent's
         number is the yardstick).
  host:  pmx_sponge_squeeze_bytes_batch on page-locked buffers against pmx_sponge_squeeze_batch + pmx_from_mont + the byte cut in numpy
         (wall clock, median).
Every form is checked on a sample of sponges against oracle/cref and Python integers before it is timed.  Prints one JSON line.
usage: python tools/squeeze_bytes_rate.py [--steps 20] [--baseline-library PATH] [--native-only]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sponge_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--baseline-library", default=None)
ap.add_argument("--native-only", action="store_true", help="only the native squeeze (what the child process of --baseline-library runs)")
ap.add_argument("--library", default=None, help="bind this build of the library (an older one may lack the new entry points)")
ARGS = ap.parse_args()
if ARGS.library:
    _lib.use_library(os.path.abspath(ARGS.library), older_build=True)

import sponge_amd as S  # noqa: E402
from sponge_amd import synth  # noqa: E402
from oracle import cref  # noqa: E402
from oracle import poseidon_oracle as O  # noqa: E402

DEV = torch.device("cuda", 0)
WARMUP = 3
SAMPLE = 256


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.int32)).to(DEV)


def step_times(fn):
    """ms of every step of fn on the current stream (HIP events around each step), after a warm-up"""
    stream = torch.cuda.current_stream()
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(ARGS.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def cut_bytes(p, elements, length, bits):
    """src/poseidon/mod.rs:256-286 in Python integers"""
    rinv = pow(1 << 256, -1, p)
    ubits = p.bit_length() - 1
    rows = []
    for row in elements:
        acc = []
        for e in row:
            x = int.from_bytes(e.tobytes(), "little") * rinv % p
            acc += [(x >> j) & 1 for j in range(ubits)] if bits else list(x.to_bytes(32, "little")[:ubits // 8])
        rows.append(acc[:length])
    return np.array(rows, dtype=np.uint8)


def run(label, field, p, bits, rate, log_n, seed):
    rp = 57 if rate == 8 else 31
    cfg = S.poseidon_config_from_lfsr(field, rate, 5, 8, rp)
    ctx, t, n = cfg.context(0), rate + 1, 1 << log_n
    st = torch.cuda.current_stream().cuda_stream
    states = synth.random_elements(field, n * t, seed=seed).reshape(n, t, 4)
    d_st0, d_tag0, d_idx0 = dev(states), torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    d_st, d_tag, d_idx = d_st0.clone(), d_tag0.clone(), d_idx0.clone()
    d_el = torch.zeros((n, 2, 4), dtype=torch.int64, device=DEV)

    def reset():
        d_st.copy_(d_st0), d_tag.copy_(d_tag0), d_idx.copy_(d_idx0)

    def native():
        reset()
        ctx.sponge_squeeze_batch_dev(d_st.data_ptr(), d_tag.data_ptr(), d_idx.data_ptr(), d_el.data_ptr(), 2, n, st)

    ms_reset = float(np.median(step_times(reset)))
    t_native = step_times(native)
    res = {"config": label, "sponges": n, "reset_ms": round(ms_reset, 4), "native_squeeze_ms": round(float(np.median(t_native)) - ms_reset, 4),
           "native_squeeze_ms_min": round(min(t_native) - ms_reset, 4)}
    if ARGS.native_only:
        return res

    cr = cref.CRef(O.make_config(p, bits, rate, 5, 8, rp))
    rng = np.random.default_rng(seed)
    sample = np.sort(rng.choice(n, SAMPLE, replace=False))
    want_el = cr.permute_batch(states[sample], threads=0)[:, cfg.capacity:cfg.capacity + 2]
    d_bytes = torch.zeros((n, 32), dtype=torch.uint8, device=DEV)
    d_bits = torch.zeros((n, 256), dtype=torch.uint8, device=DEV)

    def as_bytes():
        reset()
        ctx.sponge_squeeze_bytes_batch_dev(d_st.data_ptr(), d_tag.data_ptr(), d_idx.data_ptr(), d_bytes.data_ptr(), 32, n, st)

    def as_bits():
        reset()
        ctx.sponge_squeeze_bits_batch_dev(d_st.data_ptr(), d_tag.data_ptr(), d_idx.data_ptr(), d_bits.data_ptr(), 256, n, st)

    as_bytes(), as_bits()
    torch.cuda.synchronize()
    assert np.array_equal(d_bytes.cpu().numpy()[sample], cut_bytes(p, want_el, 32, False)), label
    assert np.array_equal(d_bits.cpu().numpy()[sample], cut_bytes(p, want_el, 256, True)), label
    ms_bytes = float(np.median(step_times(as_bytes))) - ms_reset
    ms_bits = float(np.median(step_times(as_bits))) - ms_reset
    res.update({"squeeze_bytes_32_ms": round(ms_bytes, 4), "squeeze_bits_256_ms": round(ms_bits, 4),
                "bytes_over_native_this_build": round(ms_bytes / res["native_squeeze_ms"], 3),
                "bits_over_native_this_build": round(ms_bits / res["native_squeeze_ms"], 3)})
    del d_bytes, d_bits, d_el

    # the host entries on page-locked buffers: before (native squeeze, from_mont, numpy cut) and after
    modulus = np.array([(p >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
    h_st = S.pinned_empty((n, t, 4))
    h_el = S.pinned_empty((n, 2, 4))
    h_words = S.pinned_empty((n * 2 // 8 + 1, 1, 4))      # tag and index words, page-locked too
    h_tag = h_words.reshape(-1).view(np.uint32)[:n]
    h_idx = h_words.reshape(-1).view(np.uint32)[n:2 * n]
    h_out = S.pinned_empty((n, 1, 4)).reshape(-1).view(np.uint8).reshape(n, 32)
    L = _lib.lib()
    ub = (p.bit_length() - 1) // 8

    def fill():
        h_st[:] = states
        h_tag[:] = 0
        h_idx[:] = 0

    def before():
        _lib.check(L.pmx_sponge_squeeze_batch(ctx._h, h_st.ctypes.data, h_tag.ctypes.data, h_idx.ctypes.data, h_el.ctypes.data, 2, n))
        _lib.check(L.pmx_from_mont(modulus.ctypes.data, h_el.ctypes.data, n * 2))
        return np.ascontiguousarray(h_el.view(np.uint8).reshape(n, 2, 32)[:, :, :ub].reshape(n, 2 * ub)[:, :32])

    def after():
        _lib.check(L.pmx_sponge_squeeze_bytes_batch(ctx._h, h_st.ctypes.data, h_tag.ctypes.data, h_idx.ctypes.data, h_out.ctypes.data, 32, n))
        return h_out

    times = {"before": [], "after": []}
    outs = {}
    for rep in range(2 + min(ARGS.steps, 7)):
        for name, fn in (("before", before), ("after", after)):
            fill()
            t0 = time.perf_counter()
            outs[name] = fn().copy() if rep == 0 else fn()
            if rep >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
            if rep == 0:
                first = outs[name]
                assert np.array_equal(first[sample], cut_bytes(p, want_el, 32, False)), (label, name)
    res.update({"host_native_then_from_mont_then_cut_ms": round(float(np.median(times["before"])), 3),
                "host_native_then_from_mont_then_cut_ms_min_max": [round(min(times["before"]), 3), round(max(times["before"]), 3)],
                "host_squeeze_bytes_ms": round(float(np.median(times["after"])), 3),
                "host_squeeze_bytes_ms_min_max": [round(min(times["after"]), 3), round(max(times["after"]), 3)],
                "host_speedup": round(float(np.median(times["before"]) / np.median(times["after"])), 2)})
    return res


def main():
    shapes = [("bls12_381_fr t=3 a=5", S.BLS12_381_FR, O.BLS12_381_FR, 255, 2, 20, 0x5B11),
              ("bn254_fr t=9 a=5", S.BN254_FR, O.BN254_FR, 254, 8, 18, 0x5B19)]
    out = {"tool": "squeeze_bytes_rate", "steps": ARGS.steps, "warmup": WARMUP, "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(_lib.library_path())}
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        out["clocks"] = [ln.strip() for ln in smi.splitlines() if "sclk" in ln or "mclk" in ln][:2]   # (read-only query)
    except Exception as e:   # the tool is optional on a box without it
        out["clocks"] = "unavailable: %s" % type(e).__name__
    out["results"] = [run(*s) for s in shapes]
    if ARGS.baseline_library and not ARGS.native_only:
        torch.cuda.synchronize()
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(ARGS.steps), "--native-only", "--library",
                                ARGS.baseline_library], capture_output=True, text=True, timeout=900)
        assert child.returncode == 0, child.stderr[-2000:]
        base = json.loads(child.stdout.strip().splitlines()[-1])
        out["baseline_library"] = base
        for r, b in zip(out["results"], base["results"]):
            r["baseline_native_squeeze_ms"] = b["native_squeeze_ms"]
            r["bytes_over_baseline_native"] = round(r["squeeze_bytes_32_ms"] / b["native_squeeze_ms"], 3)
            r["bits_over_baseline_native"] = round(r["squeeze_bits_256_ms"] / b["native_squeeze_ms"], 3)
            r["targets"] = {"bytes": 1.10, "bits": 1.25}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
