"""Variable-length rows (pmx_hash_varlen_batch_dev, pmx_sponge_absorb_varlen_batch_dev) against what a caller can do with the fixed
drivers: BLS12-381 Fr t = 3 alpha = 5 at 2^20 rows and BN254 Fr t = 9 at 2^18 rows, device-resident, HIP events after a warm-up.
  (a) the ragged hash at one uniform length L = 4 rate, against pmx_hash_batch_dev on the same rows
  (b) the ragged hash with lengths uniform in [1, 8 rate], against bucketing: one pmx_hash_batch_dev per distinct length, the rows
      gathered into and the digests scattered out of each bucket by torch indexing (the index lists are precomputed, not timed)
  (c) the same as (b) for the absorb on sponges in random modes: ragged absorb against one pmx_sponge_absorb_batch_dev per bucket
Rates are permutations the reference executes per second (src/poseidon/mod.rs:121-150, 232-254, 321-341), counted on the host from the
lengths and modes.  Every form is checked on a sample of rows against oracle/cref before it is timed.  Prints one JSON line.
usage: python tools/varlen_rate.py [reps, default 10]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sponge_amd as S  # noqa: E402
from sponge_amd import synth  # noqa: E402
from oracle import cref  # noqa: E402
from oracle import poseidon_oracle as O  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
DEV = torch.device("cuda", 0)
SAMPLE = 256


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.int32)).to(DEV)


def host(t: torch.Tensor, dtype=np.uint64) -> np.ndarray:
    return t.cpu().numpy().view(dtype)


def absorb_perms(tag, idx, lens, rate):
    """permutations of absorb(len) per sponge in mode (tag, idx): the up-front one (Squeezing, or a full rate), then one per rate
    filled with input left (vectorised form of mod.rs:232-254, 121-150)"""
    lens = lens.astype(np.int64)
    first = (tag != S.MODE_ABSORBING) | (idx == rate)
    i0 = np.where(first, 0, idx).astype(np.int64)
    more = np.maximum(lens - (rate - i0), 0)
    return np.where(lens == 0, 0, first.astype(np.int64) + (more + rate - 1) // rate)


def timed(fn):
    stream = torch.cuda.current_stream()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(REPS):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def run(label, field, p, bits, rate, log_n, seed):
    cfg = S.poseidon_config_from_lfsr(field, rate, 5, 8, 57 if rate == 8 else 31)
    cr = cref.CRef(O.make_config(p, bits, rate, 5, 8, 57 if rate == 8 else 31))
    ctx, t, n = cfg.context(0), rate + 1, 1 << log_n
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(seed)
    sample = rng.choice(n, SAMPLE, replace=False)
    res = {"config": label, "rows": n}

    # (a) uniform length: ragged vs fixed
    L = 4 * rate
    msgs = synth.random_elements(field, n * L, seed=seed)
    d_msgs, d_off_u = dev(msgs), dev(np.arange(n + 1, dtype=np.uint64) * L)
    d_out_r = torch.zeros((n, 1, 4), dtype=torch.int64, device=DEV)
    d_out_f = torch.zeros_like(d_out_r)
    ragged_u = lambda: ctx.hash_varlen_batch_dev(d_msgs.data_ptr(), d_off_u.data_ptr(), L, d_out_r.data_ptr(), 1, n, st)
    fixed_u = lambda: ctx.hash_batch_dev(d_msgs.data_ptr(), L, d_out_f.data_ptr(), 1, n, st)
    ragged_u(), fixed_u()
    torch.cuda.synchronize()
    want = cr.hash_batch(msgs.reshape(n, L, 4)[sample], L, 1, threads=0)
    assert np.array_equal(host(d_out_r).reshape(n, 1, 4)[sample], want) and torch.equal(d_out_r, d_out_f), label
    perms_u = int(n * ((L - 1) // rate + 1))   # per row: ceil(L / rate) - 1 in the absorb from Absorbing{0}, 1 in the squeeze
    ms_r, ms_f = timed(ragged_u), timed(fixed_u)
    res["uniform"] = {"len": L, "ragged_ms": round(ms_r, 4), "fixed_ms": round(ms_f, 4), "ragged_over_fixed": round(ms_f / ms_r, 3),
                      "fixed_perms_per_s": perms_u / ms_f * 1e3}
    del d_msgs, d_out_f

    # (b) lengths uniform in [1, 8 rate]: ragged vs bucketing
    lens = rng.integers(1, 8 * rate + 1, n).astype(np.uint64)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    elems = synth.random_elements(field, int(offsets[-1]), seed=seed + 1)
    d_el, d_off = dev(elems), dev(offsets)
    buckets = []
    for Lb in np.unique(lens):
        rows = np.nonzero(lens == Lb)[0]
        gather = (offsets[rows][:, None] + np.arange(int(Lb), dtype=np.uint64)[None, :]).reshape(-1).astype(np.int64)
        buckets.append((int(Lb), len(rows), torch.from_numpy(rows.astype(np.int64)).to(DEV), torch.from_numpy(gather).to(DEV)))
    d_out_b = torch.zeros((n, 1, 4), dtype=torch.int64, device=DEV)

    def bucketed_hash():
        for Lb, cnt, rows, gather in buckets:
            inp = d_el.index_select(0, gather)
            out = torch.empty((cnt, 1, 4), dtype=torch.int64, device=DEV)
            ctx.hash_batch_dev(inp.data_ptr(), Lb, out.data_ptr(), 1, cnt, st)
            d_out_b.index_copy_(0, rows, out)

    ragged_h = lambda: ctx.hash_varlen_batch_dev(d_el.data_ptr(), d_off.data_ptr(), 8 * rate, d_out_r.data_ptr(), 1, n, st)
    ragged_h(), bucketed_hash()
    torch.cuda.synchronize()
    got = host(d_out_r).reshape(n, 1, 4)
    for i in sample[:64]:
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        assert np.array_equal(got[i], cr.hash_batch(elems[lo:hi].reshape(1, hi - lo, 4), hi - lo, 1)[0]), (label, i)
    assert torch.equal(d_out_r, d_out_b), label
    perms_h = int(((lens.astype(np.int64) - 1) // rate + 1).sum())   # per row: ceil(len / rate) - 1 in the absorb, 1 in the squeeze
    ms_r, ms_b = timed(ragged_h), timed(bucketed_hash)
    res["random_hash"] = {"len": [1, 8 * rate], "buckets": len(buckets), "ragged_ms": round(ms_r, 4), "bucketed_ms": round(ms_b, 4),
                          "ragged_perms_per_s": perms_h / ms_r * 1e3, "bucketed_perms_per_s": perms_h / ms_b * 1e3,
                          "ragged_over_bucketed": round(ms_b / ms_r, 3),
                          "ragged_over_fixed_perm_rate": round((perms_h / ms_r) / (perms_u / res["uniform"]["fixed_ms"]), 3)}
    del d_out_b

    # (c) the absorb on sponges in random modes: ragged vs bucketing (each timed rep starts from the same states)
    states = synth.random_elements(field, n * t, seed=seed + 2).reshape(n, t, 4)
    tag = rng.integers(0, 2, n).astype(np.uint32)
    idx = rng.integers(0, rate + 1, n).astype(np.uint32)
    d_st0, d_tag0, d_idx0 = dev(states), dev(tag), dev(idx)
    d_st, d_tag, d_idx = d_st0.clone(), d_tag0.clone(), d_idx0.clone()

    def reset():
        d_st.copy_(d_st0), d_tag.copy_(d_tag0), d_idx.copy_(d_idx0)

    def ragged_a():
        reset()
        ctx.sponge_absorb_varlen_batch_dev(d_st.data_ptr(), d_tag.data_ptr(), d_idx.data_ptr(), d_el.data_ptr(), d_off.data_ptr(),
                                           8 * rate, n, st)

    def bucketed_a():
        reset()
        for Lb, cnt, rows, gather in buckets:
            inp = d_el.index_select(0, gather)
            s, tg, ix = d_st.index_select(0, rows), d_tag.index_select(0, rows), d_idx.index_select(0, rows)
            ctx.sponge_absorb_batch_dev(s.data_ptr(), tg.data_ptr(), ix.data_ptr(), inp.data_ptr(), Lb, cnt, st)
            d_st.index_copy_(0, rows, s), d_tag.index_copy_(0, rows, tg), d_idx.index_copy_(0, rows, ix)

    ragged_a()
    torch.cuda.synchronize()
    r_st, r_tag, r_idx = d_st.clone(), d_tag.clone(), d_idx.clone()
    bucketed_a()
    torch.cuda.synchronize()
    assert torch.equal(r_st, d_st) and torch.equal(r_tag, d_tag) and torch.equal(r_idx, d_idx), label
    g_st, g_tag, g_idx = host(r_st).reshape(n, t, 4), host(r_tag, np.uint32), host(r_idx, np.uint32)
    for i in sample[:64]:
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        w = cr.sponge_absorb(states[i], int(tag[i]), int(idx[i]), elems[lo:hi])
        assert np.array_equal(g_st[i], w[0]) and (int(g_tag[i]), int(g_idx[i])) == w[1:], (label, i)
    perms_a = int(absorb_perms(tag, idx, lens, rate).sum())
    ms_reset = timed(reset)
    ms_r, ms_b = timed(ragged_a) - ms_reset, timed(bucketed_a) - ms_reset
    res["random_absorb"] = {"len": [1, 8 * rate], "ragged_ms": round(ms_r, 4), "bucketed_ms": round(ms_b, 4),
                            "ragged_perms_per_s": perms_a / ms_r * 1e3, "bucketed_perms_per_s": perms_a / ms_b * 1e3,
                            "ragged_over_bucketed": round(ms_b / ms_r, 3)}
    return res


def main():
    out = {"tool": "varlen_rate", "reps": REPS, "device": torch.cuda.get_device_name(0), "results": [
        run("bls12_381_fr t=3 a=5", S.BLS12_381_FR, O.BLS12_381_FR, 255, 2, 20, 0x7A11),
        run("bn254_fr t=9 a=5", S.BN254_FR, O.BN254_FR, 254, 8, 18, 0x7A19),
    ]}
    for r in out["results"]:
        for k in ("uniform", "random_hash", "random_absorb"):
            for m, v in r[k].items():
                if m.endswith("per_s"):
                    r[k][m] = float("%.4g" % v)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
