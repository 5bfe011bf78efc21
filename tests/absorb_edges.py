"""Absorbed elements chosen from the state they meet - TEST INFRASTRUCTURE.

Every absorbed element reaches a sponge's state through one field addition, `state[capacity + i] += element`
(reference src/poseidon/mod.rs:128,143).  The kernels do that addition on the ABI residues (x * 2^256 mod p) in
two ways - lazily in the per-lane kernels, reduced later by the next permutation or by the conversion back to the
ABI form; with one exact conditional subtraction in the pass kernels - and a random element almost never makes
the sum land on p, p +- 1 or 2p - 2, where a reduction that is off by one subtraction would show.

`EdgeSponges` steps n sponges in lockstep with the reference's semantics (absorb mod.rs:232-254 + 121-150,
squeeze mod.rs:321-341 + 153-182), permuting through the C port in batches, and picks element k of a sponge
from the residue `s` at `state[capacity + idx]` at that moment:
    "sum_p"     x = p - s          (s != 0)      raw sum p
    "sum_pm1"   x = p - 1 - s                    raw sum p - 1
    "sum_pp1"   x = p + 1 - s      (s >= 2)      raw sum p + 1
    "x_zero"    x = 0
    "x_pm1"     x = p - 1                        (raw sum 2p - 2 when s = p - 1: recorded as "sum_2pm2" as well)
    "random"    now and then
All values are raw residues - the limbs the ABI carries and the kernels add.  The tracked states, mode words and
squeeze outputs are the reference's: the GPU tests compare with them and, sponge by sponge, with the C port."""
from __future__ import annotations

import random

import numpy as np

from oracle import cref
from oracle import poseidon_oracle as O

TARGETS = ("sum_p", "sum_pm1", "sum_pp1", "x_zero", "x_pm1")
ALL_HITS = TARGETS + ("random", "sum_2pm2")
ABSORBING, SQUEEZING = 0, 1
_M64 = (1 << 64) - 1


def to_ints(arr: np.ndarray):
    """[..., 4] u64 limbs -> flat list of Python ints"""
    a = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4)
    return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in a]


def to_limbs(vals) -> np.ndarray:
    return np.array([[(v >> (64 * i)) & _M64 for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def edge_states(p: int, n: int, t: int, seed: int) -> np.ndarray:
    """[n][t][4] start states whose lanes are mostly 0, 1, p - 2 or p - 1 (values only a caller can put into a state), some random"""
    rng = random.Random(seed)
    vals = [rng.choice((0, 1, p - 2, p - 1, p - 1, rng.randrange(p))) for _ in range(n * t)]
    return to_limbs(vals).reshape(n, t, 4)


def mixed_modes(n: int, rate: int, seed: int):
    """mode words of every kind, neighbours in different modes: Absorbing{0..rate}, Squeezing{0..rate}"""
    rng = np.random.default_rng(seed)
    tag = rng.integers(0, 2, n).astype(np.uint32)
    idx = rng.integers(0, rate + 1, n).astype(np.uint32)
    return tag, idx


class EdgeSponges:
    """n sponges of one config (an oracle.poseidon_oracle.PoseidonConfig), stepped in lockstep.

    fresh=True: rows of the hash driver (new sponges); until a sponge's first permutation its elements are 0 or p - 1 only.
    hits[target] counts the additions made for each target; `adds` keeps (call, sponge, element, s, x, target) of every one."""

    def __init__(self, ocfg: O.PoseidonConfig, states=None, tag=None, idx=None, n=None, seed=0, fresh=False, c_port=None):
        self.cfg, self.p = ocfg, ocfg.p
        self.t, self.rate, self.cap = ocfg.t, ocfg.rate, ocfg.capacity
        if states is None:
            states = np.zeros((n, self.t, 4), dtype=np.uint64)
        self.state = np.ascontiguousarray(states, dtype=np.uint64).copy()
        self.n = self.state.shape[0]
        self.tag = np.zeros(self.n, np.uint32) if tag is None else np.asarray(tag, np.uint32).copy()
        self.idx = np.zeros(self.n, np.uint32) if idx is None else np.asarray(idx, np.uint32).copy()
        self.cr = c_port or cref.CRef(ocfg)
        self.rng = random.Random(seed)
        self.count = [self.rng.randrange(len(TARGETS)) for _ in range(self.n)]   # per-sponge position in the target cycle
        self.fresh = np.full(self.n, bool(fresh))
        self.hits = {k: 0 for k in ALL_HITS}
        self.adds = []
        self.calls = 0
        self.permutations = 0

    def _permute(self, rows) -> None:
        rows = np.asarray(rows)
        if rows.size:
            self.state[rows] = self.cr.permute_batch(np.ascontiguousarray(self.state[rows]), threads=0)
            self.fresh[rows] = False
            self.permutations += int(rows.size)

    def _choose(self, i: int, s: int):
        p = self.p
        if self.fresh[i]:
            x = (p - 1) if self.rng.random() < 0.5 else 0
            return x, ("x_pm1" if x else "x_zero")
        if self.rng.random() < 0.12:
            return self.rng.randrange(p), "random"
        if s == p - 1 and self.rng.random() < 0.5:      # a caller-set top lane: the raw sum 2p - 2
            return p - 1, "x_pm1"
        for _ in range(len(TARGETS)):
            target = TARGETS[self.count[i] % len(TARGETS)]
            self.count[i] += 1
            if target == "sum_p" and s != 0:
                return p - s, target
            if target == "sum_pm1":
                return p - 1 - s, target
            if target == "sum_pp1" and s >= 2:
                return p + 1 - s, target
            if target == "x_zero":
                return 0, target
            if target == "x_pm1":
                return p - 1, target
        raise AssertionError("unreachable: x_zero is always possible")

    def absorb(self, length: int) -> np.ndarray:
        """absorb(length) on every sponge: returns the elements [n][length][4] and advances the tracked sponges"""
        n, p = self.n, self.p
        elems = np.zeros((n, length, 4), dtype=np.uint64)
        self.calls += 1
        if length == 0:
            return elems                                                        # mod.rs:234-236: no-op
        cur = np.where(self.tag == ABSORBING, np.minimum(self.idx, self.rate), self.rate).astype(np.int64)
        rows = np.arange(n)
        for j in range(length):
            self._permute(np.nonzero(cur == self.rate)[0])                      # rate full and more input (mod.rs:137-148, 241-252)
            cur[cur == self.rate] = 0
            pos = self.cap + cur
            svals = to_ints(self.state[rows, pos])
            xs, sums = [], []
            for i in range(n):
                s = svals[i]
                x, target = self._choose(i, s)
                assert 0 <= x < p
                self.hits[target] += 1
                if s == p - 1 and x == p - 1:
                    self.hits["sum_2pm2"] += 1
                self.adds.append((self.calls - 1, i, j, s, x, target))
                xs.append(x)
                sums.append((s + x) % p)                                        # field addition of the residues
            elems[:, j] = to_limbs(xs)
            self.state[rows, pos] = to_limbs(sums)
            cur += 1
        self.tag[:] = ABSORBING
        self.idx[:] = cur
        return elems

    def squeeze(self, length: int) -> np.ndarray:
        """squeeze_native_field_elements(length) on every sponge: returns [n][length][4]"""
        n, rate, cap = self.n, self.rate, self.cap
        out = np.zeros((n, length, 4), dtype=np.uint64)
        self.calls += 1
        start = np.where(self.tag == SQUEEZING, np.minimum(self.idx, rate), 0).astype(np.int64)
        pending = (self.tag != SQUEEZING) | (start == rate)                     # mod.rs:324-336
        start[pending] = 0
        rem = np.full(n, length, dtype=np.int64)
        pos = np.zeros(n, dtype=np.int64)
        active = np.ones(n, dtype=bool)
        while active.any():
            self._permute(np.nonzero(active & pending)[0])
            pending[:] = False
            for i in np.nonzero(active)[0]:
                s0, r = int(start[i]), int(rem[i])
                if s0 + r <= rate:                                              # squeeze_internal, mod.rs:153-182
                    out[i, pos[i]:pos[i] + r] = self.state[i, cap + s0:cap + s0 + r]
                    self.idx[i] = s0 + r
                    active[i] = False
                    continue
                take = rate - s0
                out[i, pos[i]:pos[i] + take] = self.state[i, cap + s0:cap + rate]
                pending[i] = r != rate                                          # mod.rs:175, before the slice advances
                rem[i] -= take
                pos[i] += take
                start[i] = 0
        self.tag[:] = SQUEEZING
        return out


def hash_rows(ocfg: O.PoseidonConfig, n: int, in_len: int, out_len: int, seed: int, c_port=None):
    """rows of the hash driver (new; absorb(in_len); squeeze_native(out_len)) whose elements meet the edges: (msgs, digests)"""
    g = EdgeSponges(ocfg, n=n, seed=seed, fresh=True, c_port=c_port)
    msgs = g.absorb(in_len)
    return msgs, g.squeeze(out_len), g


def oracle_sums(ocfg: O.PoseidonConfig, start_state, tag, idx, script, elems_by_call, picks):
    """Recompute, with the pure-Python oracle, the raw sum s + x of the additions `picks` = [(call, element)] of ONE sponge.
    script: [("absorb" | "squeeze", length)], elems_by_call[c]: that sponge's elements of call c (canonical ints of residues).
    Returns {(call, element): s + x} with s read from the oracle's state (as a residue) at the moment of the addition."""
    p = ocfg.p
    sp = O.PoseidonSponge(ocfg, [O.from_mont(v, p) for v in start_state], int(tag), int(idx))
    want = set(picks)
    got = {}
    for c, (op, length) in enumerate(script):
        if op == "squeeze":
            sp.squeeze_native_field_elements(length)
            continue
        for j in range(length):
            x = elems_by_call[c][j]
            if (c, j) in want:
                probe = sp.clone()
                if probe.mode != O.ABSORBING or probe.index == ocfg.rate:
                    probe._permute()
                    at = 0
                else:
                    at = probe.index
                got[(c, j)] = O.to_mont(probe.state[ocfg.capacity + at], p) + x
            sp.absorb([O.from_mont(x, p)])                                       # absorbing one by one = absorbing the block
    return got
