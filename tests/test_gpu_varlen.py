"""Variable-length rows for the batch hash and absorb drivers (pmx_hash_varlen_batch[_dev], pmx_sponge_absorb_varlen_batch[_dev]):
every row a length of its own, on every engine - the quad engine (t = 3, <= 32768 sponges), the window engines as passes (t = 3 from
32769 sponges, t = 4 .. 9), the run-time-width engine (t = 2, t >= 10).  Reference semantics: new :219-230, absorb :232-254 with
absorb_internal :121-150, squeeze_native_field_elements :321-341 (src/poseidon/mod.rs); every sponge / row is checked against the C
restatement (oracle/cref), the large hashes per length bucket with its threaded hash_batch."""
import ctypes

import numpy as np
import pytest
import torch

import sponge_amd as S
from sponge_amd import _lib, synth
from oracle import cref
from oracle import poseidon_oracle as O

pytestmark = pytest.mark.gpu

FIELD = {"bls": (S.BLS12_381_FR, O.BLS12_381_FR, 255), "bn254": (S.BN254_FR, O.BN254_FR, 254)}


def _config(field, rate, alpha, rf, rp):
    f, p, bits = FIELD[field]
    return f, S.poseidon_config_from_lfsr(f, rate, alpha, rf, rp), cref.CRef(O.make_config(p, bits, rate, alpha, rf, rp))


def _engine(cfg, n, length):
    info = _lib.PmxEngineInfo()
    _lib.check(_lib.lib().pmx_ctx_engine_info(cfg.context()._h, _lib.OP_ABSORB, n, length, ctypes.byref(info)))
    return info.engine


def _lengths(n, r, rng, top=5):
    """0, 1, r-1, r, r+1, 2r and random values up to top * r"""
    base = [0, 1, max(r - 1, 0), r, r + 1, 2 * r]
    lens = rng.integers(0, top * r + 1, n)
    lens[:len(base) * 4] = np.tile(base, 4)[:min(n, len(base) * 4)]
    return lens.astype(np.uint64)


def _rows(f, lens, seed, skip=0):
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens) + skip
    offsets[0] = skip
    elems = synth.random_elements(f, int(offsets[-1]) + 1, seed=seed)[:int(offsets[-1])]
    return np.ascontiguousarray(elems), offsets


def _modes(n, r, rng):
    tag = rng.integers(0, 2, n).astype(np.uint32)
    idx = rng.integers(0, r + 1, n).astype(np.uint32)
    # empty rows on the sponges a non-empty absorb would permute first: Squeezing{rate}, Absorbing{rate}, Squeezing{0}
    tag[[0, 1, 2]] = [S.MODE_SQUEEZING, S.MODE_ABSORBING, S.MODE_SQUEEZING]
    idx[[0, 1, 2]] = [r, r, 0]
    return tag, idx


def _check_absorb(f, cfg, cr, n, r, seed):
    rng = np.random.default_rng(seed)
    lens = _lengths(n, r, rng)
    lens[:3] = 0
    elems, offsets = _rows(f, lens, seed)
    batch = S.BatchPoseidonSponge.new(cfg, n)
    batch.state = synth.random_elements(f, n * cfg.t, seed=seed + 1).reshape(n, cfg.t, 4)
    batch.mode_tag, batch.mode_index = _modes(n, r, rng)
    before = batch.clone()
    batch.absorb_varlen(elems, offsets)
    for i in range(n):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        if lo == hi:   # untouched, whatever the mode (mod.rs:234-236)
            assert np.array_equal(batch.state[i], before.state[i]) and batch.mode_tag[i] == before.mode_tag[i] \
                and batch.mode_index[i] == before.mode_index[i], i
            continue
        st, m, ix = cr.sponge_absorb(before.state[i], int(before.mode_tag[i]), int(before.mode_index[i]), elems[lo:hi])
        assert np.array_equal(batch.state[i], st) and (int(batch.mode_tag[i]), int(batch.mode_index[i])) == (m, ix), (i, hi - lo)
    return lens


def _check_hash(f, cfg, cr, n, r, seed, out_len=3):
    rng = np.random.default_rng(seed)
    lens = _lengths(n, r, rng)
    elems, offsets = _rows(f, lens, seed)
    got = cfg.context().hash_varlen_batch(elems, offsets, out_len)
    for L in np.unique(lens):
        rows = np.nonzero(lens == L)[0]
        msgs = np.stack([elems[int(offsets[i]):int(offsets[i + 1])] for i in rows]).reshape(len(rows), int(L), 4)
        want = cr.hash_batch(msgs, int(L), out_len, threads=0) if L else cr.hash_batch(np.zeros((len(rows), 0, 4), dtype=np.uint64), 0, out_len)
        assert np.array_equal(got[rows], want), int(L)
    # an empty row hashes like pmx_hash_batch with in_len = 0
    empty = cfg.context().hash_batch(np.zeros((1, 0, 4), dtype=np.uint64), 0, out_len, n=1)
    assert np.array_equal(got[np.nonzero(lens == 0)[0][0]], empty[0])


# (label, field, rate, alpha, RF, RP, n, engine expected)
ENGINES = [
    ("quad-t3", "bls", 2, 5, 8, 31, 1000, b"QuadEngine"),
    ("window-t3", "bls", 2, 5, 8, 31, 32769 + 300, b"HybridEngine<3,5"),
    ("t4", "bls", 3, 5, 8, 56, 589, b"HybridEngine<4,5"),
    ("t5", "bls", 4, 5, 8, 56, 589, b"HybridEngine<5,5"),
    ("t6", "bls", 5, 5, 8, 57, 589, b"HybridEngine<6,5"),
    ("t7", "bls", 6, 5, 8, 57, 589, b"HybridEngine<7,5"),
    ("t8", "bls", 7, 5, 8, 57, 589, b"HybridEngine<8,5"),
    ("t9-bn254", "bn254", 8, 5, 8, 57, 589, b"HybridEngine<9,5"),
    ("t9-alpha17", "bls", 8, 17, 8, 57, 589, b"HybridEngine<9,0"),   # (any exponent but 5: the generic S-box build)
    ("lds-t2", "bls", 1, 5, 8, 31, 589, b"LdsEngine<5>"),
    ("lds-t10", "bls", 9, 5, 8, 57, 589, b"LdsEngine<5>"),
]


@pytest.mark.parametrize("case", ENGINES, ids=lambda c: c[0])
def test_varlen_absorb_and_hash_on_every_engine(case):
    label, field, rate, alpha, rf, rp, n, engine = case
    f, cfg, cr = _config(field, rate, alpha, rf, rp)
    assert _engine(cfg, n, 5 * rate).startswith(engine), (_engine(cfg, n, 5 * rate), engine)
    if engine.startswith(b"HybridEngine"):
        assert b"passes" in _engine(cfg, n, 5 * rate)
    _check_absorb(f, cfg, cr, n, rate, seed=100 + rate + alpha)
    _check_hash(f, cfg, cr, n, rate, seed=200 + rate + alpha)


@pytest.mark.parametrize("label,field,rate,n", [("quad-t3", "bls", 2, 700), ("window-t3", "bls", 2, 40000), ("t9", "bn254", 8, 700)])
def test_uniform_lengths_are_bit_identical_to_the_fixed_driver(label, field, rate, n):
    f, cfg, cr = _config(field, rate, 5, 8, 57 if rate == 8 else 31)
    ctx = cfg.context()
    rng = np.random.default_rng(rate)
    for L in (1, rate, rate + 1, 3 * rate + 1):
        msgs = synth.random_elements(f, n * L, seed=L).reshape(n, L, 4)
        offsets = np.arange(n + 1, dtype=np.uint64) * L
        assert np.array_equal(ctx.hash_varlen_batch(msgs.reshape(-1, 4), offsets, 2), ctx.hash_batch(msgs, L, 2)), L
        a = S.BatchPoseidonSponge.new(cfg, n)
        a.state = synth.random_elements(f, n * cfg.t, seed=50 + L).reshape(n, cfg.t, 4)
        a.mode_tag, a.mode_index = _modes(n, rate, rng)
        b = a.clone()
        a.absorb_varlen(msgs.reshape(-1, 4), offsets)
        b.absorb(msgs)
        assert np.array_equal(a.state, b.state) and np.array_equal(a.mode_tag, b.mode_tag) and np.array_equal(a.mode_index, b.mode_index)


def test_shuffling_rows_permutes_the_results():
    f, cfg, cr = _config("bls", 2, 5, 8, 31)
    ctx = cfg.context()
    rng = np.random.default_rng(7)
    for n in (900, 40000):
        lens = _lengths(n, 2, rng)
        elems, offsets = _rows(f, lens, seed=n)
        rows = [elems[int(offsets[i]):int(offsets[i + 1])] for i in range(n)]
        perm = rng.permutation(n)
        got = ctx.hash_varlen_batch(rows, None, 2)
        shuffled = ctx.hash_varlen_batch([rows[i] for i in perm], None, 2)
        assert np.array_equal(shuffled, got[perm])
        st = synth.random_elements(f, n * 3, seed=n + 1).reshape(n, 3, 4)
        tag, idx = _modes(n, 2, rng)
        a = S.BatchPoseidonSponge.from_state((st, tag, idx), cfg)
        b = S.BatchPoseidonSponge.from_state((st[perm], tag[perm], idx[perm]), cfg)
        a.absorb_varlen(rows)
        b.absorb_varlen([rows[i] for i in perm])
        assert np.array_equal(b.state, a.state[perm]) and np.array_equal(b.mode_tag, a.mode_tag[perm]) \
            and np.array_equal(b.mode_index, a.mode_index[perm])


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.int32)).to("cuda:0")


def _host(t: torch.Tensor, dtype=np.uint64) -> np.ndarray:
    return t.cpu().numpy().view(dtype)


@pytest.mark.parametrize("field,rate,n", [("bls", 2, 500), ("bls", 2, 40000), ("bn254", 8, 700), ("bls", 1, 300)])
def test_dev_entries_on_torch_tensors(field, rate, n):
    """offsets[0] != 0 (the rows start behind 11 other elements of the buffer), and a row longer than max_len: absorbed up to max_len
    elements"""
    f, cfg, cr = _config(field, rate, 5, 8, 57 if rate == 8 else 31)
    ctx = cfg.context()
    rng = np.random.default_rng(n)
    lens = _lengths(n, rate, rng, top=4)
    max_len = 4 * rate
    lens[5] = 6 * rate + 1                 # longer than max_len: clamped
    elems, offsets = _rows(f, lens, seed=n + 3, skip=11)
    clamped = np.minimum(lens, max_len)
    stream = torch.cuda.current_stream().cuda_stream
    d_in, d_off = _dev(elems), _dev(offsets)
    # absorb
    st = synth.random_elements(f, n * cfg.t, seed=n + 4).reshape(n, cfg.t, 4)
    tag, idx = _modes(n, rate, rng)
    d_st, d_tag, d_idx = _dev(st), _dev(tag), _dev(idx)
    ctx.sponge_absorb_varlen_batch_dev(d_st.data_ptr(), d_tag.data_ptr(), d_idx.data_ptr(), d_in.data_ptr(), d_off.data_ptr(), max_len, n, stream)
    torch.cuda.synchronize()
    got_st, got_tag, got_idx = _host(d_st).reshape(n, cfg.t, 4), _host(d_tag, np.uint32), _host(d_idx, np.uint32)
    for i in range(n):
        lo, L = int(offsets[i]), int(clamped[i])
        if L == 0:
            assert np.array_equal(got_st[i], st[i]) and (got_tag[i], got_idx[i]) == (tag[i], idx[i]), i
            continue
        want = cr.sponge_absorb(st[i], int(tag[i]), int(idx[i]), elems[lo:lo + L])
        assert np.array_equal(got_st[i], want[0]) and (int(got_tag[i]), int(got_idx[i])) == (want[1], want[2]), (i, L)
    # hash
    d_out = torch.zeros((n, 2, 4), dtype=torch.int64, device="cuda:0")
    ctx.hash_varlen_batch_dev(d_in.data_ptr(), d_off.data_ptr(), max_len, d_out.data_ptr(), 2, n, stream)
    torch.cuda.synchronize()
    got = _host(d_out).reshape(n, 2, 4)
    for i in range(n):
        lo, L = int(offsets[i]), int(clamped[i])
        assert np.array_equal(got[i], cr.hash_batch(elems[lo:lo + L].reshape(1, L, 4), L, 2)[0]), (i, L)


def test_length_limits():
    f, cfg, cr = _config("bls", 2, 5, 8, 31)
    ctx = cfg.context()
    n, r = 64, 2
    # a _dev bound above 65536 rates: PMX_ERR_ARG, nothing launched
    st = synth.random_elements(f, n * 3, seed=5).reshape(n, 3, 4)
    tag, idx = _modes(n, r, np.random.default_rng(5))
    elems = synth.random_elements(f, n, seed=6)
    offsets = np.arange(n + 1, dtype=np.uint64)
    d_st, d_tag, d_idx, d_in, d_off = _dev(st), _dev(tag), _dev(idx), _dev(elems), _dev(offsets)
    d_out = torch.zeros((n, 1, 4), dtype=torch.int64, device="cuda:0")
    for fn, args in (("pmx_sponge_absorb_varlen_batch_dev", (d_st.data_ptr(), d_tag.data_ptr(), d_idx.data_ptr(), d_in.data_ptr(), d_off.data_ptr())),
                     ("pmx_hash_varlen_batch_dev", (d_in.data_ptr(), d_off.data_ptr()))):
        bound = 65536 * r + 1
        full = args + ((bound, n, 0) if fn.startswith("pmx_sponge") else (bound, d_out.data_ptr(), 1, n, 0))
        assert getattr(_lib.lib(), fn)(ctx._h, *full) == _lib.PMX_ERR_ARG, fn
        assert b"65536" in _lib.lib().pmx_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_st).reshape(n, 3, 4), st) and np.array_equal(_host(d_tag, np.uint32), tag)
    assert not d_out.any()
    # the host entries take any length: one row longer than 65536 rates among short rows, absorbed in pieces
    lens = np.random.default_rng(9).integers(0, 7, n).astype(np.uint64)
    lens[17] = 65536 * r + 5
    elems, offsets = _rows(f, lens, seed=10)
    batch = S.BatchPoseidonSponge.from_state((st, tag, idx), cfg)
    batch.absorb_varlen(elems, offsets)
    out = ctx.hash_varlen_batch(elems, offsets, 1)
    for i in range(n):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        if hi > lo:
            want = cr.sponge_absorb(st[i], int(tag[i]), int(idx[i]), elems[lo:hi])
            assert np.array_equal(batch.state[i], want[0]) and (int(batch.mode_tag[i]), int(batch.mode_index[i])) == want[1:], i
        assert np.array_equal(out[i], cr.hash_batch(elems[lo:hi].reshape(1, hi - lo, 4), hi - lo, 1)[0]), i


def test_host_validation_leaves_everything_unchanged():
    f, cfg, cr = _config("bls", 2, 5, 8, 31)
    n = 50
    st = synth.random_elements(f, n * 3, seed=21).reshape(n, 3, 4)
    tag, idx = _modes(n, 2, np.random.default_rng(21))
    elems = synth.random_elements(f, 3 * n, seed=22)
    offsets = np.arange(n + 1, dtype=np.uint64) * 3
    offsets[31] = offsets[30] - 1                    # row 30 ends before it starts
    batch = S.BatchPoseidonSponge.from_state((st, tag, idx), cfg)
    with pytest.raises(S.PmxError) as e:
        batch.absorb_varlen(elems, offsets)
    assert e.value.code == _lib.PMX_ERR_ARG and "row 30" in str(e.value)
    with pytest.raises(S.PmxError) as e:
        cfg.context().hash_varlen_batch(elems, offsets, 1)
    assert e.value.code == _lib.PMX_ERR_ARG and "row 30" in str(e.value)
    assert np.array_equal(batch.state, st) and np.array_equal(batch.mode_tag, tag) and np.array_equal(batch.mode_index, idx)
    bad = idx.copy()
    bad[7] = 3                                       # index above the rate
    batch = S.BatchPoseidonSponge.from_state((st, tag, bad), cfg)
    with pytest.raises(S.PmxError) as e:
        batch.absorb_varlen(elems, np.arange(n + 1, dtype=np.uint64) * 3)
    assert e.value.code == _lib.PMX_ERR_ARG and "sponge 7" in str(e.value)
    assert np.array_equal(batch.state, st) and np.array_equal(batch.mode_index, bad)


@pytest.mark.parametrize("field,rate,log_n", [("bls", 2, 20), ("bn254", 8, 18)])
def test_full_size_ragged_hash(field, rate, log_n):
    """2^20 BLS12-381 t = 3 rows and 2^18 BN254 t = 9 rows, lengths uniform in [1, 8 rate], device-resident; every row checked"""
    f, cfg, cr = _config(field, rate, 5, 8, 57 if rate == 8 else 31)
    n = 1 << log_n
    lens = np.random.default_rng(log_n).integers(1, 8 * rate + 1, n).astype(np.uint64)
    elems, offsets = _rows(f, lens, seed=log_n)
    d_in, d_off = _dev(elems), _dev(offsets)
    d_out = torch.zeros((n, 1, 4), dtype=torch.int64, device="cuda:0")
    cfg.context().hash_varlen_batch_dev(d_in.data_ptr(), d_off.data_ptr(), 8 * rate, d_out.data_ptr(), 1, n,
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = _host(d_out).reshape(n, 1, 4)
    for L in np.unique(lens):
        rows = np.nonzero(lens == L)[0]
        idx = offsets[rows][:, None] + np.arange(int(L), dtype=np.uint64)[None, :]
        msgs = elems[idx.reshape(-1).astype(np.int64)].reshape(len(rows), int(L), 4)
        assert np.array_equal(got[rows], cr.hash_batch(msgs, int(L), 1, threads=0)), int(L)
