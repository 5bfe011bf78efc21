"""The Poseidon permutation walked BACKWARDS, to plant chosen values inside it  --  TEST INFRASTRUCTURE ONLY.

With gcd(alpha, p - 1) = 1 the S-box x -> x^alpha is a bijection whose inverse is x -> x^(alpha^-1 mod p - 1), the Cauchy MDS matrix is
invertible, and adding a round constant is undone by subtracting it: a state chosen at any round boundary can be walked back to the input
that produces it.  tests/plants.py uses this to make the device meet 0, 1, p - 1 and their kin in every round; it never takes an
expected value from here (those come from the C port), and checks every plant with trace() below, the forward walk of
oracle/poseidon_oracle.permute with its intermediate values kept.

Python integers throughout, canonical values in [0, p); nothing of the library under test is imported.  The batch forms keep a set of
states as a numpy object array [t][n] so that a layer is one matrix product.  The one costly step is the root, an exponent as long as
the modulus (about 120 us with pow()): powers() hands batches of them to oracle/modpow.c, compiled on demand into a temporary
directory as cref.native_lib does, and falls back to pow() where that cannot be built.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import poseidon_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))


# ----------------------------------------------------------------------------------------------
# The two inverses
# ----------------------------------------------------------------------------------------------
def alpha_inverse(cfg: O.PoseidonConfig) -> int:
    """d with (x^alpha)^d = x for every x of the field; raises where x -> x^alpha is no bijection"""
    g = math.gcd(cfg.alpha, cfg.p - 1)
    if g != 1:
        raise ValueError("gcd(alpha = %d, p - 1) = %d: the S-box is not invertible" % (cfg.alpha, g))
    return pow(cfg.alpha, -1, cfg.p - 1)


def mds_inverse(cfg: O.PoseidonConfig) -> List[List[int]]:
    """Gauss-Jordan mod p"""
    p, t = cfg.p, cfg.t
    a = [[v % p for v in row] + [int(i == j) for j in range(t)] for i, row in enumerate(cfg.mds)]
    for col in range(t):
        pivot = next((r for r in range(col, t) if a[r][col]), None)
        if pivot is None:
            raise ValueError("the MDS matrix is singular")
        a[col], a[pivot] = a[pivot], a[col]
        scale = pow(a[col][col], -1, p)
        a[col] = [v * scale % p for v in a[col]]
        for r in range(t):
            if r != col and a[r][col]:
                f = a[r][col]
                a[r] = [(v - f * w) % p for v, w in zip(a[r], a[col])]
    return [row[t:] for row in a]


def is_full_round(cfg: O.PoseidonConfig, rnd: int) -> bool:
    half = cfg.full_rounds // 2
    return rnd < half or rnd >= half + cfg.partial_rounds


# ----------------------------------------------------------------------------------------------
# x^e mod p for many x
# ----------------------------------------------------------------------------------------------
_modpow = None


def modpow_lib():
    """oracle/modpow.c built with the machine's C compiler into a private temporary directory, or None"""
    global _modpow
    if _modpow is None:
        import shutil
        import subprocess
        import tempfile
        _modpow = False
        cc = shutil.which("gcc") or shutil.which("cc")
        if cc:
            out = os.path.join(tempfile.mkdtemp(prefix="pmx_oracle_modpow_"), "libmodpow.so")
            try:
                subprocess.check_call([cc, "-O2", "-fPIC", "-std=c11", "-shared", "-o", out, os.path.join(HERE, "modpow.c")],
                                      stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
                h = ctypes.CDLL(out)
                h.modpow_batch.restype = ctypes.c_int
                h.modpow_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_uint64]
                _modpow = h
            except Exception:
                _modpow = False
    return _modpow or None


def powers(xs: Sequence[int], e: int, p: int, use_c: bool = True) -> List[int]:
    """[x^e mod p for x in xs], every x in [0, p)"""
    xs = [int(x) for x in xs]
    h = modpow_lib() if use_c and len(xs) >= 8 and p % 2 and p.bit_length() <= 255 and 0 <= e < 1 << 256 else None
    if h is None:
        return [pow(x, e, p) for x in xs]
    from concurrent.futures import ThreadPoolExecutor
    buf = np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype=np.uint64).copy()
    consts = [np.array(O.to_limbs(v), dtype=np.uint64) for v in (e, p, (1 << 512) % p)]
    inv = (-pow(p, -1, 1 << 64)) % (1 << 64)
    n, workers = len(xs), min(8, len(os.sched_getaffinity(0)))
    step = max(64, -(-n // workers))

    def some(first):
        count = min(step, n - first)
        h.modpow_batch(ctypes.c_void_p(buf.ctypes.data + 32 * first), count, *(ctypes.c_void_p(c.ctypes.data) for c in consts), inv)
    with ThreadPoolExecutor(workers) as pool:                                  # (ctypes releases the GIL)
        list(pool.map(some, range(0, n, step)))
    raw = buf.tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n)]


def _apply(fn, arr: np.ndarray) -> np.ndarray:
    """fn (list of ints -> list of ints) on every element of an object array"""
    out = np.empty(arr.size, dtype=object)
    out[:] = fn(list(arr.reshape(-1)))
    return out.reshape(arr.shape)


def _obj(rows) -> np.ndarray:
    a = np.empty((len(rows), len(rows[0])), dtype=object)
    for i, row in enumerate(rows):
        a[i, :] = [int(v) for v in row]
    return a


# ----------------------------------------------------------------------------------------------
# Backwards
# ----------------------------------------------------------------------------------------------
def back_to_many(cfg: O.PoseidonConfig, planted: Sequence[Tuple[int, Sequence[int]]]) -> List[List[int]]:
    """planted: (r, state) pairs, `state` the state at the START of round r, before its ARK (r = R_f + R_p: the output).  Returns the
    permutation's input of each, in order.  One walk from the output down to round 0 serves all of them: a state joins at its round."""
    p, t = cfg.p, cfg.t
    total = cfg.full_rounds + cfg.partial_rounds
    d = alpha_inverse(cfg)
    minv = _obj(mds_inverse(cfg))
    joining: Dict[int, List[int]] = {}
    for k, (r, state) in enumerate(planted):
        assert 0 <= r <= total and len(state) == t and all(0 <= int(v) < p for v in state)
        joining.setdefault(r, []).append(k)
    order: List[int] = []
    s = np.empty((t, 0), dtype=object)
    for r in range(total, -1, -1):
        if r in joining:
            order += joining[r]
            s = np.concatenate([s, _obj([planted[k][1] for k in joining[r]]).T], axis=1)
        if r == 0 or not order:
            continue
        rnd = r - 1                                             # undo round rnd: MDS, S-box, ARK
        s = minv.dot(s) % p
        if is_full_round(cfg, rnd):
            s = _apply(lambda xs: powers(xs, d, p), s)
        else:
            s[0] = _apply(lambda xs: powers(xs, d, p), s[0])
        s = (s - _obj([cfg.ark[rnd]]).T) % p
    out: List[List[int]] = [[]] * len(planted)
    for col, k in enumerate(order):
        out[k] = [int(v) for v in s[:, col]]
    return out


def back_to(cfg: O.PoseidonConfig, state: Sequence[int], r: int) -> List[int]:
    """the input x for which the state at the start of round r (before its ARK) is `state`; r = R_f + R_p: permute(x) == state"""
    return back_to_many(cfg, [(r, state)])[0]


# ----------------------------------------------------------------------------------------------
# Forwards, keeping what every round saw
# ----------------------------------------------------------------------------------------------
def trace_many(cfg: O.PoseidonConfig, xs: Sequence[Sequence[int]]):
    """(sbox_in, sbox_out, out): object arrays [R][t][n], [R][t][n], [t][n] - per round the state after ARK (lane 0 alone enters the
    S-box in a partial round) and the state after the S-box layer (in a partial round lanes 1 .. t - 1 pass unchanged), and the output.
    The round loop of oracle/poseidon_oracle.permute."""
    p, t, alpha = cfg.p, cfg.t, cfg.alpha
    total = cfg.full_rounds + cfg.partial_rounds
    mds = _obj(cfg.mds)
    s = _obj(xs).T
    n = s.shape[1]
    sbox_in = np.empty((total, t, n), dtype=object)
    sbox_out = np.empty((total, t, n), dtype=object)
    for rnd in range(total):
        s = (s + _obj([cfg.ark[rnd]]).T) % p                                # apply_ark
        sbox_in[rnd] = s
        s = s.copy()
        if is_full_round(cfg, rnd):                                         # full round
            s = _apply(lambda v: [pow(x, alpha, p) for x in v], s)
        else:                                                               # partial
            s[0] = _apply(lambda v: [pow(x, alpha, p) for x in v], s[0])
        sbox_out[rnd] = s
        s = mds.dot(s) % p                                                  # apply_mds
    return sbox_in, sbox_out, s


def trace(cfg: O.PoseidonConfig, x: Sequence[int]):
    """(sbox_in [R][t], sbox_out [R][t], out [t]) of one input, as lists of integers"""
    a, b, out = trace_many(cfg, [list(x)])
    return ([[int(v) for v in r[:, 0]] for r in a], [[int(v) for v in r[:, 0]] for r in b], [int(v) for v in out[:, 0]])
